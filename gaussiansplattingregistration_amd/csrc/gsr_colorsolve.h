// gsr_colorsolve.h -- the joint colour fit over a graph of scenes (gsr_color_solve, include/gsr_hip.h).
// Plain C++ (no HIP include, nothing of the library): csrc/harmonize.hip wraps it, and scripts/colorsolve_selftest.cpp compiles it
// under a sanitizer.  Graphs have tens of nodes: one dense system of d (free nodes) unknowns, d = 1, 3 or 12.
//
// A node's transform is P = sum_k theta_k B_k over the mode's basis of 3 x 4 matrices (gain: [I|0]; channel gain: e_c e_c^T; affine:
// e_c e_j^T).  With the bilinear forms  AA(X, Y) = sum_c x^c' S_aa y^c,  AB(X, Y) = sum_c x^c' S_ab y^c,  BB(X, Y) = sum_c x^c' S_bb y^c
// (x^c = row c of X) an edge costs  AA(Ps, Ps) - 2 AB(Ps, Pt) + BB(Pt, Pt),  so the normal equations H theta = g are
//   H[sk, sl] += AA(B_k, B_l)   H[tk, tl] += BB(B_k, B_l)   H[sk, tl] -= AB(B_k, B_l)   (and its transpose)
//   g[sk] += AB(B_k, Pt) for a held t,   g[tl] += AB(Ps, B_l) for a held s,
// and the prior lambda |P - [I|0]|_F^2 adds lambda <B_k, B_l> to H and lambda <B_k, [I|0]> to g.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "gsr_posegraph.h"      // ldlt_pivoted, fmt: the n x n diagonal-pivoted LDL^T

namespace gsr {
namespace colorsolve {

constexpr int SUMS_LEN = 40;
enum Mode { GAIN = 0, CHANNEL_GAIN = 1, AFFINE = 2 };

struct Edge {
    int s = 0, t = 0;
    double sums[SUMS_LEN];
};
struct Result {
    double E_initial = 0, E_final = 0, pivot_min = 0, pivot_max = 0;
    int n_free = 0, n_unknowns = 0;
};

// the three 4 x 4 blocks of an edge's sums, S_aa and S_bb filled out from their upper triangles
struct Blocks {
    double aa[16], ab[16], bb[16];
    explicit Blocks(const double* sums) {
        int k = 3;
        for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) { aa[4 * i + j] = aa[4 * j + i] = sums[k++]; }
        for (int i = 0; i < 16; ++i) ab[i] = sums[k++];
        for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) { bb[4 * i + j] = bb[4 * j + i] = sums[k++]; }
    }
};
// sum_c x^c' S y^c for two 3 x 4 matrices
inline double form(const double* S, const double* X, const double* Y) {
    double e = 0;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 4; ++i) {
            if (X[4 * c + i] == 0.0) continue;          // the basis matrices are sparse
            double t = 0;
            for (int j = 0; j < 4; ++j) t += S[4 * i + j] * Y[4 * c + j];
            e += X[4 * c + i] * t;
        }
    return e;
}

inline int mode_dim(int mode) { return mode == GAIN ? 1 : mode == CHANNEL_GAIN ? 3 : mode == AFFINE ? 12 : 0; }
inline void basis(int mode, int k, double* B) {
    for (int i = 0; i < 12; ++i) B[i] = 0.0;
    if (mode == GAIN) B[0] = B[5] = B[10] = 1.0;
    else if (mode == CHANNEL_GAIN) B[5 * k] = 1.0;
    else B[k] = 1.0;
}

inline double objective(int n_nodes, const double* P, const std::vector<Edge>& edges, const std::vector<char>& held, double lambda) {
    double E = 0;
    for (const Edge& e : edges) {
        const Blocks S(e.sums);
        const double *Ps = P + 12 * e.s, *Pt = P + 12 * e.t;
        E += form(S.aa, Ps, Ps) - 2.0 * form(S.ab, Ps, Pt) + form(S.bb, Pt, Pt);
    }
    for (int i = 0; i < n_nodes; ++i) {
        if (held[i]) continue;
        double q = 0;
        for (int k = 0; k < 12; ++k) { const double d = P[12 * i + k] - (k % 5 == 0 ? 1.0 : 0.0); q += d * d; }
        E += lambda * q;
    }
    return E;
}

// P: n_nodes x 12 in and out; held: one per node or NULL.  Returns "" or the error message.
inline std::string solve(int n_nodes, double* P, const std::vector<Edge>& edges, int mode, double prior, int64_t min_pairs, int reference,
                         int32_t* held_out, Result* result) {
    using posegraph::fmt;
    auto finite = [](double v) { return fabs(v) <= 1.79e308; };
    if (n_nodes < 1 || !P) return "no nodes";
    const int d = mode_dim(mode);
    if (d == 0) return fmt("unknown mode %g", mode);
    if (!(prior >= 0.0) || !finite(prior)) return fmt("prior %g is negative or not finite", prior);
    if (reference < 0 || reference >= n_nodes) return fmt("reference %g is outside [0, %g)", reference, n_nodes);
    for (int i = 0; i < n_nodes; ++i)
        for (int k = 0; k < 12; ++k)
            if (!finite(P[12 * i + k])) return fmt("transform of node %g is not finite", i);
    double sum_w = 0;
    for (size_t k = 0; k < edges.size(); ++k) {
        const Edge& e = edges[k];
        if (e.s < 0 || e.s >= n_nodes || e.t < 0 || e.t >= n_nodes) return fmt("edge %g: node index out of range (%g, %g)", (double)k, e.s, e.t);
        if (e.s == e.t) return fmt("edge %g: source == target (%g)", (double)k, e.s);
        for (int i = 0; i < SUMS_LEN; ++i) if (!finite(e.sums[i])) return fmt("edge %g: sum %g is not finite", (double)k, i);
        sum_w += e.sums[1];
    }
    const double lambda = edges.empty() ? 0.0 : prior * sum_w / (double)edges.size();

    // held: the reference, and what no path of edges with n >= min_pairs connects to it
    std::vector<char> held(n_nodes, 1);
    {
        std::vector<char> seen(n_nodes, 0);
        std::vector<int> queue(1, reference);
        seen[reference] = 1;
        for (size_t h = 0; h < queue.size(); ++h)
            for (const Edge& e : edges) {
                if (!(e.sums[0] >= (double)min_pairs)) continue;
                const int other = e.s == queue[h] ? e.t : (e.t == queue[h] ? e.s : -1);
                if (other >= 0 && !seen[other]) { seen[other] = 1; queue.push_back(other); }
            }
        for (int i = 0; i < n_nodes; ++i) held[i] = !seen[i] || i == reference;
    }
    std::vector<int> var(n_nodes, -1);
    int n_free = 0;
    for (int i = 0; i < n_nodes; ++i) if (!held[i]) var[i] = d * n_free++;
    const int n = d * n_free;

    Result res;
    res.n_free = n_free;
    res.n_unknowns = n;
    res.E_initial = objective(n_nodes, P, edges, held, lambda);
    if (n > 0) {
        std::vector<double> B((size_t)d * 12);
        for (int k = 0; k < d; ++k) basis(mode, k, &B[12 * (size_t)k]);
        const double I0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        std::vector<double> H((size_t)n * n, 0.0), g(n, 0.0);
        for (const Edge& e : edges) {
            const Blocks S(e.sums);
            const int vs = var[e.s], vt = var[e.t];
            for (int k = 0; k < d; ++k) {
                const double* Bk = &B[12 * (size_t)k];
                for (int l = 0; l < d; ++l) {
                    const double* Bl = &B[12 * (size_t)l];
                    if (vs >= 0) H[(size_t)(vs + k) * n + vs + l] += form(S.aa, Bk, Bl);
                    if (vt >= 0) H[(size_t)(vt + k) * n + vt + l] += form(S.bb, Bk, Bl);
                    if (vs >= 0 && vt >= 0) {
                        const double v = form(S.ab, Bk, Bl);
                        H[(size_t)(vs + k) * n + vt + l] -= v;
                        H[(size_t)(vt + l) * n + vs + k] -= v;
                    }
                }
                if (vs >= 0 && vt < 0) g[vs + k] += form(S.ab, Bk, P + 12 * e.t);
                if (vt >= 0 && vs < 0) g[vt + k] += form(S.ab, P + 12 * e.s, Bk);
            }
        }
        for (int i = 0; i < n_free; ++i)
            for (int k = 0; k < d; ++k) {
                for (int l = 0; l < d; ++l) {
                    double q = 0;
                    for (int m = 0; m < 12; ++m) q += B[12 * (size_t)k + m] * B[12 * (size_t)l + m];
                    H[(size_t)(d * i + k) * n + d * i + l] += lambda * q;
                }
                double q = 0;
                for (int m = 0; m < 12; ++m) q += B[12 * (size_t)k + m] * I0[m];
                g[d * i + k] += lambda * q;
            }
        double dmax = 0;
        for (int i = 0; i < n; ++i) dmax = fmax(dmax, H[(size_t)i * n + i]);
        std::vector<int> perm;
        const int rank = posegraph::ldlt_pivoted(n, H, perm, 1e-12 * dmax);
        if (rank != n)
            return fmt("the system of %g unknowns is singular to rounding (rank %g): the pairs do not determine this mode's transform; raise prior", n, rank);
        res.pivot_min = res.pivot_max = H[0];
        for (int i = 1; i < n; ++i) { res.pivot_min = fmin(res.pivot_min, H[(size_t)i * n + i]); res.pivot_max = fmax(res.pivot_max, H[(size_t)i * n + i]); }
        std::vector<double> y(n);
        for (int i = 0; i < n; ++i) {
            double s = g[perm[i]];
            for (int j = 0; j < i; ++j) s -= H[(size_t)i * n + j] * y[j];
            y[i] = s;
        }
        for (int i = 0; i < n; ++i) y[i] /= H[(size_t)i * n + i];
        for (int i = n - 1; i >= 0; --i) {
            double s = y[i];
            for (int j = i + 1; j < n; ++j) s -= H[(size_t)j * n + i] * y[j];
            y[i] = s;
        }
        std::vector<double> theta(n);
        for (int i = 0; i < n; ++i) theta[perm[i]] = y[i];
        for (int i = 0; i < n; ++i) if (!finite(theta[i])) return "the solution is not finite; raise prior";
        for (int i = 0; i < n_nodes; ++i) {
            if (var[i] < 0) continue;                   // a held node's twelve doubles are never written
            for (int m = 0; m < 12; ++m) {
                double v = 0;
                for (int k = 0; k < d; ++k) v += theta[var[i] + k] * B[12 * (size_t)k + m];
                P[12 * i + m] = v;
            }
        }
    }
    res.E_final = objective(n_nodes, P, edges, held, lambda);
    if (held_out) for (int i = 0; i < n_nodes; ++i) held_out[i] = held[i];
    if (result) *result = res;
    return "";
}

}  // namespace colorsolve
}  // namespace gsr
