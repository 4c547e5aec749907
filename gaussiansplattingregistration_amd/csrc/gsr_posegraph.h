// gsr_posegraph.h -- pose-graph optimisation of a multiway registration (gsr_posegraph_optimize, include/gsr_hip.h): the SO(3) log / exp,
// the edge residual and its analytic Jacobians, Levenberg-Marquardt with the line process in closed form, pruning, the connectivity
// check.  Plain C++ (no HIP include, nothing of the library): csrc/posegraph.hip wraps it, and a stand-alone host program can compile it
// under a sanitizer.  Graphs have tens of nodes: one dense 6 (N - 1) system per step.
//
// Frames.  X_i maps node i's frame into the global one; an edge's T maps the source's frame into the target's; consistent: X_t T = X_s.
// Residual.  D = X_t^-1 X_s T^-1 (the left perturbation in the TARGET frame, the frame the information matrix of the pair is written
// in), r = [log_SO3(R_D); t_D], chi = r^T Lambda r -- to first order sum_q |D q - q|^2 over the pair's correspondences.
// Increment.  X_i <- X_i [exp(w) | v] (right, in the node's own frame).  With phi = log R_D:
//     dr / d(w, v)_t = [ -Jl^-1(phi)      0 ]        dr / d(w, v)_s = [ Jr^-1(phi) R_T         0       ]
//                      [  [t_D]x         -I ]                         [ R_D [t_T]x R_T      R_D R_T   ]
// Objective (Choi, Zhou, Koltun 2015) with the line process eliminated: a certain edge costs chi, an uncertain one mu chi / (mu + chi);
// its weight l = (mu / (mu + chi))^2 is the derivative of that cost, so Gauss-Newton with the weights of the current poses has the
// objective's exact gradient.  gsr_solve.h's pivoted LDL^T is a fixed 6x6 unrolled for the device and lives behind a HIP include; the
// same algorithm (diagonal pivoting) is written here for n x n and used for the damped system and for the semi-definiteness check.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

namespace gsr {
namespace posegraph {

struct Edge {
    int s = 0, t = 0;
    bool uncertain = false;
    double T[16];
    double info[36];
};
struct Option {
    double max_correspondence_distance = 0.075, edge_prune_threshold = 0.25, preference_loop_closure = 1.0;
    int reference_node = 0, max_iteration = 100, max_iteration_lm = 20;
    double min_relative_increment = 1e-6, min_relative_residual_increment = 1e-6, min_right_term = 1e-6, min_residual = 1e-6;
};
struct Result {
    int iterations[2] = {0, 0};
    int n_pruned = 0;
    double E_initial = 0, E_final = 0, mu = 0, mu_first = 0;
};

// ---- 3x3 (row-major double[9]) and rigid 4x4 (row-major double[16], rows 0..2 used) ------------------------------------------------
inline void mul3(const double* A, const double* B, double* C) {
    double R[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    for (int i = 0; i < 9; ++i) C[i] = R[i];
}
inline void skew(const double* v, double* S) {
    S[0] = 0; S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2]; S[4] = 0; S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0]; S[8] = 0;
}
inline void rigid_mul(const double* A, const double* B, double* C) {        // C = A B
    double R[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) R[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j];
        R[4 * i + 3] += A[4 * i + 3];
    }
    R[12] = R[13] = R[14] = 0; R[15] = 1;
    for (int i = 0; i < 16; ++i) C[i] = R[i];
}
inline void rigid_inv(const double* A, double* C) {                        // [R | t]^-1 = [R^T | -R^T t]
    double R[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[4 * i + j] = A[4 * j + i];
        R[4 * i + 3] = -(A[i] * A[3] + A[4 + i] * A[7] + A[8 + i] * A[11]);
    }
    R[12] = R[13] = R[14] = 0; R[15] = 1;
    for (int i = 0; i < 16; ++i) C[i] = R[i];
}

inline void so3_exp(const double* w, double* R) {                         // Rodrigues
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double a, b;                                                          // R = I + a [w]x + b [w]x^2
    if (th < 1e-4) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    double S[9], S2[9];
    skew(w, S);
    mul3(S, S, S2);
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * S[i] + b * S2[i];
}
inline void so3_log(const double* R, double* w) {
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};      // sin(theta) * axis
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double th = atan2(s, c);
    if (th < 1e-6) { const double k = 1.0 + th * th / 6.0; w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2]; return; }
    if (c > -0.99) { const double k = th / s; w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2]; return; }
    // near pi the antisymmetric part vanishes: the axis from the diagonal, R_ii = c + (1 - c) a_i^2, its signs from v (or, at pi
    // itself, from the symmetric off-diagonal entries relative to the largest component)
    double a[3];
    for (int i = 0; i < 3; ++i) { const double d = (R[4 * i] - c) / (1.0 - c); a[i] = d > 0 ? sqrt(d) : 0.0; }
    int m = a[0] >= a[1] ? (a[0] >= a[2] ? 0 : 2) : (a[1] >= a[2] ? 1 : 2);
    for (int i = 0; i < 3; ++i)
        if (i != m && R[3 * m + i] + R[3 * i + m] < 0) a[i] = -a[i];
    if (a[0] * v[0] + a[1] * v[1] + a[2] * v[2] < 0) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; }
    const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int i = 0; i < 3; ++i) w[i] = th * a[i] / n;
}
// the inverse left (sign -1) / right (sign +1) Jacobian of SO(3) at phi: I + sign/2 [phi]x + c2 [phi]x^2
inline void so3_jinv(const double* phi, double sign, double* J) {
    const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], th = sqrt(th2);
    const double c2 = th < 1e-4 ? 1.0 / 12.0 + th2 / 720.0 : 1.0 / th2 - cos(0.5 * th) / (2.0 * th * sin(0.5 * th));
    double S[9], S2[9];
    skew(phi, S);
    mul3(S, S, S2);
    for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0 ? 1.0 : 0.0) + 0.5 * sign * S[i] + c2 * S2[i];
}

inline double quad6(const double* L, const double* r) {
    double s = 0;
    for (int i = 0; i < 6; ++i) { double t = 0; for (int j = 0; j < 6; ++j) t += L[6 * i + j] * r[j]; s += r[i] * t; }
    return s;
}

// residual of an edge at the poses Xs, Xt; optionally the 6x6 Jacobians (row-major) with respect to the increments of s and of t
inline void edge_residual(const Edge& e, const double* Xs, const double* Xt, double* r, double* Js = nullptr, double* Jt = nullptr) {
    double Xti[16], Ti[16], D[16];
    rigid_inv(Xt, Xti);
    rigid_inv(e.T, Ti);
    rigid_mul(Xti, Xs, D);
    rigid_mul(D, Ti, D);
    const double RD[9] = {D[0], D[1], D[2], D[4], D[5], D[6], D[8], D[9], D[10]};
    const double tD[3] = {D[3], D[7], D[11]};
    so3_log(RD, r);
    r[3] = tD[0]; r[4] = tD[1]; r[5] = tD[2];
    if (!Js) return;
    const double RT[9] = {e.T[0], e.T[1], e.T[2], e.T[4], e.T[5], e.T[6], e.T[8], e.T[9], e.T[10]};
    const double tT[3] = {e.T[3], e.T[7], e.T[11]};
    double Jr[9], Jl[9], A[9], B[9], C[9], S[9];
    so3_jinv(r, 1.0, Jr);
    so3_jinv(r, -1.0, Jl);
    mul3(Jr, RT, A);                    // d phi / d w_s
    skew(tT, S);
    mul3(S, RT, B);
    mul3(RD, B, B);                     // d t / d w_s
    mul3(RD, RT, C);                    // d t / d v_s
    skew(tD, S);                        // d t / d w_t
    for (int i = 0; i < 36; ++i) Js[i] = Jt[i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Js[6 * i + j] = A[3 * i + j];
            Js[6 * (3 + i) + j] = B[3 * i + j];
            Js[6 * (3 + i) + 3 + j] = C[3 * i + j];
            Jt[6 * i + j] = -Jl[3 * i + j];
            Jt[6 * (3 + i) + j] = S[3 * i + j];
            Jt[6 * (3 + i) + 3 + j] = i == j ? -1.0 : 0.0;
        }
}

// ---- n x n LDL^T with diagonal pivoting (Eigen's LDLT; gsr_solve.h's solve6 is its fixed 6 x 6) -------------------------------------
// A (row-major, symmetric) is overwritten.  tol: a pivot <= tol ends the factorisation; returns the number of pivots taken (n = full
// rank).  rest_max: the largest |entry| of what was left when it ended (the semi-definiteness check: nothing, for a semi-definite matrix).
inline int ldlt_pivoted(int n, std::vector<double>& A, std::vector<int>& perm, double tol, double* rest_max = nullptr) {
    perm.resize(n);
    for (int i = 0; i < n; ++i) perm[i] = i;
    if (rest_max) *rest_max = 0.0;
    for (int k = 0; k < n; ++k) {
        int piv = k;
        for (int i = k + 1; i < n; ++i) if (A[(size_t)i * n + i] > A[(size_t)piv * n + piv]) piv = i;
        if (piv != k) {
            for (int j = 0; j < n; ++j) { const double t = A[(size_t)k * n + j]; A[(size_t)k * n + j] = A[(size_t)piv * n + j]; A[(size_t)piv * n + j] = t; }
            for (int i = 0; i < n; ++i) { const double t = A[(size_t)i * n + k]; A[(size_t)i * n + k] = A[(size_t)i * n + piv]; A[(size_t)i * n + piv] = t; }
            const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
        }
        const double d = A[(size_t)k * n + k];
        if (!(d > tol)) {
            if (rest_max)
                for (int i = k; i < n; ++i) for (int j = k; j < n; ++j) { const double v = fabs(A[(size_t)i * n + j]); if (!(v <= *rest_max)) *rest_max = v; }
            return k;
        }
        for (int i = k + 1; i < n; ++i) {
            const double l = A[(size_t)i * n + k] / d;
            for (int j = k + 1; j <= i; ++j) A[(size_t)i * n + j] -= l * A[(size_t)k * n + j];       // row k still holds the column's values
            A[(size_t)i * n + k] = l;
        }
        for (int i = k + 1; i < n; ++i) for (int j = i + 1; j < n; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i];    // keep it symmetric: the pivot search and swaps read both halves
    }
    return n;
}
// x = A^-1 b for a symmetric positive definite A; false when a pivot is not positive
inline bool ldlt_solve(int n, const std::vector<double>& A_, const std::vector<double>& b, std::vector<double>& x) {
    std::vector<double> A(A_);
    std::vector<int> perm;
    if (ldlt_pivoted(n, A, perm, 0.0) != n) return false;
    std::vector<double> y(n);
    for (int i = 0; i < n; ++i) {
        double s = b[perm[i]];
        for (int j = 0; j < i; ++j) s -= A[(size_t)i * n + j] * y[j];
        y[i] = s;
    }
    for (int i = 0; i < n; ++i) y[i] /= A[(size_t)i * n + i];
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i];
        for (int j = i + 1; j < n; ++j) s -= A[(size_t)j * n + i] * y[j];
        y[i] = s;
    }
    x.assign(n, 0.0);
    for (int i = 0; i < n; ++i) x[perm[i]] = y[i];
    for (int i = 0; i < n; ++i) if (!(fabs(x[i]) <= 1.79e308)) return false;
    return true;
}

inline std::string fmt(const char* f, double a = 0, double b = 0, double c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, f, a, b, c);
    return buf;
}

// "" when the arguments are a valid problem, else the message
inline std::string validate(int n_nodes, const double* poses, const std::vector<Edge>& edges, const Option& o) {
    auto finite = [](double v) { return fabs(v) <= 1.79e308; };
    if (n_nodes < 1 || !poses) return "no nodes";
    if (!(o.max_correspondence_distance > 0) || !finite(o.max_correspondence_distance)) return fmt("option: max_correspondence_distance %g is not positive", o.max_correspondence_distance);
    if (!(o.edge_prune_threshold >= 0 && o.edge_prune_threshold <= 1)) return fmt("option: edge_prune_threshold %g is outside [0, 1]", o.edge_prune_threshold);
    if (!(o.preference_loop_closure > 0) || !finite(o.preference_loop_closure)) return fmt("option: preference_loop_closure %g is not positive", o.preference_loop_closure);
    if (o.reference_node < 0 || o.reference_node >= n_nodes) return fmt("option: reference_node %g is outside [0, %g)", o.reference_node, n_nodes);
    if (o.max_iteration < 0 || o.max_iteration_lm < 1) return fmt("option: max_iteration %g must be >= 0 and max_iteration_lm %g >= 1", o.max_iteration, o.max_iteration_lm);
    for (double v : {o.min_relative_increment, o.min_relative_residual_increment, o.min_right_term, o.min_residual})
        if (!(v >= 0) || !finite(v)) return fmt("option: a convergence threshold (%g) is negative or not finite", v);
    for (int i = 0; i < n_nodes; ++i)
        for (int k = 0; k < 16; ++k)
            if (!finite(poses[16 * i + k])) return fmt("pose of node %g is not finite", i);
    for (size_t k = 0; k < edges.size(); ++k) {
        const Edge& e = edges[k];
        if (e.s < 0 || e.s >= n_nodes || e.t < 0 || e.t >= n_nodes) return fmt("edge %g: node index out of range (%g, %g)", (double)k, e.s, e.t);
        if (e.s == e.t) return fmt("edge %g: source == target (%g)", (double)k, e.s);
        for (int i = 0; i < 16; ++i) if (!finite(e.T[i])) return fmt("edge %g: transform is not finite", (double)k);
        double mx = 0;
        for (int i = 0; i < 36; ++i) { if (!finite(e.info[i])) return fmt("edge %g: information matrix is not finite", (double)k); mx = fmax(mx, fabs(e.info[i])); }
        const double tol = 1e-9 * mx;
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < i; ++j)
                if (fabs(e.info[6 * i + j] - e.info[6 * j + i]) > tol) return fmt("edge %g: information matrix is not symmetric", (double)k);
        std::vector<double> A(e.info, e.info + 36);
        std::vector<int> perm;
        double rest = 0;
        ldlt_pivoted(6, A, perm, 6 * tol, &rest);       // a semi-definite matrix ends with nothing left beside its positive pivots
        if (rest > 36 * tol) return fmt("edge %g: information matrix is not positive semi-definite", (double)k);
    }
    // every node must be reachable from the reference node over the edges (either direction)
    std::vector<char> seen(n_nodes, 0);
    std::vector<int> queue(1, o.reference_node);
    seen[o.reference_node] = 1;
    for (size_t h = 0; h < queue.size(); ++h)
        for (const Edge& e : edges) {
            const int other = e.s == queue[h] ? e.t : (e.t == queue[h] ? e.s : -1);
            if (other >= 0 && !seen[other]) { seen[other] = 1; queue.push_back(other); }
        }
    for (int i = 0; i < n_nodes; ++i)
        if (!seen[i]) return fmt("node %g cannot be reached from the reference node %g", i, o.reference_node);
    return "";
}

inline double line_weight(double mu, double chi) {
    if (!(mu > 0)) return chi > 0 ? 0.0 : 1.0;
    const double q = mu / (mu + chi);
    return q * q;
}

struct Problem {
    int n_nodes;
    const std::vector<Edge>* edges;
    std::vector<char> active;
    double mu = 0;
    int ref = 0;

    void set_mu(const Option& o) {       // preference * d^2 * mean over the active uncertain edges of Lambda[5][5]
        double s = 0; int n = 0;
        for (size_t k = 0; k < edges->size(); ++k)
            if (active[k] && (*edges)[k].uncertain) { s += (*edges)[k].info[35]; ++n; }
        mu = n ? o.preference_loop_closure * o.max_correspondence_distance * o.max_correspondence_distance * s / n : 0.0;
    }
    double chi(size_t k, const std::vector<double>& X) const {
        const Edge& e = (*edges)[k];
        double r[6];
        edge_residual(e, &X[16 * e.s], &X[16 * e.t], r);
        return quad6(e.info, r);
    }
    double objective(const std::vector<double>& X) const {
        double E = 0;
        for (size_t k = 0; k < edges->size(); ++k) {
            if (!active[k]) continue;
            const double c = chi(k, X);
            E += (*edges)[k].uncertain ? (mu > 0 ? mu * c / (mu + c) : 0.0) : c;
        }
        return E;
    }
    int var(int node) const { return node == ref ? -1 : 6 * (node < ref ? node : node - 1); }
    // H = sum w J^T Lambda J, b = -sum w J^T Lambda r at the poses X (w = 1 or the line process weight there)
    void system(const std::vector<double>& X, std::vector<double>& H, std::vector<double>& b) const {
        const int n = 6 * (n_nodes - 1);
        H.assign((size_t)n * n, 0.0);
        b.assign(n, 0.0);
        for (size_t k = 0; k < edges->size(); ++k) {
            if (!active[k]) continue;
            const Edge& e = (*edges)[k];
            double r[6], J[2][36], LJ[2][36], Lr[6];
            edge_residual(e, &X[16 * e.s], &X[16 * e.t], r, J[0], J[1]);
            const double w = e.uncertain ? line_weight(mu, quad6(e.info, r)) : 1.0;
            for (int i = 0; i < 6; ++i) {
                Lr[i] = 0;
                for (int j = 0; j < 6; ++j) Lr[i] += e.info[6 * i + j] * r[j];
            }
            for (int a = 0; a < 2; ++a)
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        double s = 0;
                        for (int m = 0; m < 6; ++m) s += e.info[6 * i + m] * J[a][6 * m + j];
                        LJ[a][6 * i + j] = s;
                    }
            const int v[2] = {var(e.s), var(e.t)};
            for (int a = 0; a < 2; ++a) {
                if (v[a] < 0) continue;
                for (int i = 0; i < 6; ++i) {
                    double s = 0;
                    for (int m = 0; m < 6; ++m) s += J[a][6 * m + i] * Lr[m];
                    b[v[a] + i] -= w * s;
                }
                for (int c = 0; c < 2; ++c) {
                    if (v[c] < 0) continue;
                    for (int i = 0; i < 6; ++i)
                        for (int j = 0; j < 6; ++j) {
                            double s = 0;
                            for (int m = 0; m < 6; ++m) s += J[a][6 * m + i] * LJ[c][6 * m + j];
                            H[(size_t)(v[a] + i) * n + v[c] + j] += w * s;
                        }
                }
            }
        }
    }
    void retract(const std::vector<double>& X, const std::vector<double>& d, std::vector<double>& Y) const {
        Y = X;
        for (int i = 0; i < n_nodes; ++i) {
            const int v = var(i);
            if (v < 0) continue;                         // the reference node's pose is never written
            double R[9], Dl[16];
            so3_exp(&d[v], R);
            for (int a = 0; a < 3; ++a) { for (int c = 0; c < 3; ++c) Dl[4 * a + c] = R[3 * a + c]; Dl[4 * a + 3] = d[v + 3 + a]; }
            Dl[12] = Dl[13] = Dl[14] = 0; Dl[15] = 1;
            rigid_mul(&X[16 * i], Dl, &Y[16 * i]);
        }
    }
    double state_norm(const std::vector<double>& X) const {
        double s = 0;
        for (int i = 0; i < n_nodes; ++i) {
            if (i == ref) continue;
            const double* P = &X[16 * i];
            const double R[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
            double w[3];
            so3_log(R, w);
            s += w[0] * w[0] + w[1] * w[1] + w[2] * w[2] + P[3] * P[3] + P[7] * P[7] + P[11] * P[11];
        }
        return sqrt(s);
    }
};

// Levenberg-Marquardt as Open3D's GlobalOptimizationLevenbergMarquardt steps it: lambda_0 = 1e-5 max diag H; an accepted step scales
// lambda by max(1/3, 1 - (2 rho - 1)^3), a rejected one by ni = 2, 4, 8, ...  Returns the accepted steps.
inline int levenberg_marquardt(const Problem& P, const Option& o, std::vector<double>& X) {
    const int n = 6 * (P.n_nodes - 1);
    if (n == 0) return 0;
    std::vector<double> H, b, Hd, d, Y;
    double E = P.objective(X);
    P.system(X, H, b);
    double lambda = 0;
    for (int i = 0; i < n; ++i) lambda = fmax(lambda, H[(size_t)i * n + i]);
    lambda = lambda > 0 ? 1e-5 * lambda : 1e-5;
    double ni = 2.0;
    int accepted = 0;
    for (int it = 0; it < o.max_iteration; ++it) {
        if (E < o.min_residual) break;
        double bmax = 0;
        for (int i = 0; i < n; ++i) bmax = fmax(bmax, fabs(b[i]));
        if (bmax < o.min_right_term) break;
        bool stop = false, moved = false;
        for (int lm = 0; lm < o.max_iteration_lm; ++lm) {
            Hd = H;
            for (int i = 0; i < n; ++i) Hd[(size_t)i * n + i] += lambda;
            if (!ldlt_solve(n, Hd, b, d)) { lambda *= ni; ni *= 2; continue; }
            double dn = 0, pred = 0;
            for (int i = 0; i < n; ++i) { dn += d[i] * d[i]; pred += d[i] * (lambda * d[i] + b[i]); }
            dn = sqrt(dn);
            if (dn < o.min_relative_increment * (P.state_norm(X) + o.min_relative_increment)) { stop = true; break; }
            P.retract(X, d, Y);
            const double En = P.objective(Y);
            const double rho = (E - En) / pred;
            if (pred > 0 && rho > 0 && En == En) {
                if (E - En < o.min_relative_residual_increment * E) stop = true;
                X.swap(Y);
                E = En;
                const double u = 2 * rho - 1;
                lambda *= fmax(1.0 / 3.0, 1 - u * u * u);
                ni = 2.0;
                P.system(X, H, b);
                moved = true;
                ++accepted;
                break;
            }
            lambda *= ni;
            ni *= 2;
        }
        if (stop || !moved) break;       // !moved: no damping within max_iteration_lm descends -- a minimum to rounding
    }
    return accepted;
}

// The whole procedure.  poses: n_nodes x 16 in and out; line_process / pruned: one per edge or NULL.  Returns "" or the error message.
inline std::string optimize(int n_nodes, double* poses, const std::vector<Edge>& edges, const Option& o, double* line_process, int32_t* pruned, Result* result) {
    const std::string err = validate(n_nodes, poses, edges, o);
    if (!err.empty()) return err;
    std::vector<double> X(poses, poses + (size_t)16 * n_nodes);
    Problem P;
    P.n_nodes = n_nodes;
    P.edges = &edges;
    P.active.assign(edges.size(), 1);
    P.ref = o.reference_node;
    P.set_mu(o);
    Result res;
    res.mu_first = P.mu;
    res.E_initial = P.objective(X);
    res.iterations[0] = levenberg_marquardt(P, o, X);
    std::vector<double> l(edges.size(), 1.0);
    for (size_t k = 0; k < edges.size(); ++k) {
        if (!edges[k].uncertain) continue;
        l[k] = line_weight(P.mu, P.chi(k, X));
        if (l[k] < o.edge_prune_threshold) { P.active[k] = 0; ++res.n_pruned; }
    }
    P.set_mu(o);
    res.iterations[1] = levenberg_marquardt(P, o, X);
    for (size_t k = 0; k < edges.size(); ++k)
        if (edges[k].uncertain && P.active[k]) l[k] = line_weight(P.mu, P.chi(k, X));
    res.mu = P.mu;
    res.E_final = P.objective(X);
    for (int i = 0; i < n_nodes; ++i)
        if (i != o.reference_node)
            for (int k = 0; k < 16; ++k) poses[16 * i + k] = X[16 * i + k];
    for (size_t k = 0; k < edges.size(); ++k) {
        if (line_process) line_process[k] = l[k];
        if (pruned) pruned[k] = P.active[k] ? 0 : 1;
    }
    if (result) *result = res;
    return "";
}

}  // namespace posegraph
}  // namespace gsr
