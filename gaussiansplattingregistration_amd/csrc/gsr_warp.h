// gsr_warp.h -- the host side of non-rigid refinement: the lattice arithmetic shared with csrc/warp.hip and the
// solver behind gsr_warp_solve.  No HIP include: scripts/warp_selftest.cpp compiles this header alone under ASan / UBSan, and
// gsr_warp_solve works on a machine without a GPU (as gsr_posegraph_optimize does).
//
// The unknowns are the node displacements U (M x 3, node (ix, iy, iz) at (ix ny + iy) nz + iz).  At fixed correspondences
//   E(U) = sum_cells (S_rr + 2 b_c' u_c + u_c' A_c u_c) + wT sum_triples |U_a - 2 U_b + U_c|^2 + wE sum_edges |U_a - U_b|^2 + w0 sum |U_a|^2
// with wT = lam n_C / n_T, wE = 0.01 lam n_C / n_E, w0 = lam0 n_C / M (a term whose count is 0 is dropped) and u_c the 24-vector of the
// cell's eight nodes (local node k = 4 bx + 2 by + bz, component a at 3 k + a).  E is quadratic: H U = -b is solved once, exactly.
//
// Solver: Cholesky of the symmetric band.  A direct, backward-stable factorisation gives an error of a few units of cond(H) 2^-52,
// which is what the tests hold it to; conjugate gradients stopped at a 1e-12 residual would leave cond(H) 1e-12.  The half band is
// 3 (2 ny nz) + 2 (the second difference along x), the cost N (band)^2: 375 unknowns x 152 at 5^3 (9 Mflop), 2187 x 488 at 9^3
// (0.5 Gflop), 14739 x 1736 at 17^3 (44 Gflop, 205 MB of band: tens of seconds -- the price of the largest lattice).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

namespace gsr {
namespace warp {

constexpr int CELL_LEN = 326;      // 300 (upper triangle of sum g g', row by row) + 24 (sum g r0) + sum r0^2 + n
constexpr int MIN_DIM = 2, MAX_DIM = 17;

struct Report {
    double E_before = 0, E_after = 0;              // E at the U handed in and at the minimiser
    double E_data_before = 0, E_data_after = 0;    // the data term alone
    int64_t n_corr = 0;                            // n_C = sum of the cells' counts
    int32_t n_unknowns = 0, half_band = 0;
    double pivot_min = 0, pivot_max = 0;           // extreme diagonal entries of the Cholesky factor, squared
};

inline int tri(int a, int b) { return a * 24 - a * (a - 1) / 2 + (b - a); }      // a <= b < 24
inline bool dims_ok(const int32_t d[3]) {
    for (int a = 0; a < 3; ++a)
        if (d[a] < MIN_DIM || d[a] > MAX_DIM) return false;
    return true;
}
inline int node_of(const int32_t d[3], int ix, int iy, int iz) { return (ix * d[1] + iy) * d[2] + iz; }
inline int n_nodes(const int32_t d[3]) { return d[0] * d[1] * d[2]; }
inline int n_cells(const int32_t d[3]) { return (d[0] - 1) * (d[1] - 1) * (d[2] - 1); }
// the eight nodes of cell (cx, cy, cz) in local order
inline void cell_nodes(const int32_t d[3], int cell, int out[8]) {
    const int cz = cell % (d[2] - 1), cy = (cell / (d[2] - 1)) % (d[1] - 1), cx = cell / ((d[2] - 1) * (d[1] - 1));
    for (int k = 0; k < 8; ++k) out[k] = node_of(d, cx + (k >> 2), cy + ((k >> 1) & 1), cz + (k & 1));
}

// the regularisers as lists of (nodes, coefficients): triples (1, -2, 1) and edges (1, -1) along every axis
struct Stencil { int node[3]; int len; };
inline void stencils(const int32_t d[3], std::vector<Stencil>& triples, std::vector<Stencil>& edges) {
    const int stride[3] = {d[1] * d[2], d[2], 1};
    for (int ix = 0; ix < d[0]; ++ix)
        for (int iy = 0; iy < d[1]; ++iy)
            for (int iz = 0; iz < d[2]; ++iz) {
                const int i3[3] = {ix, iy, iz}, n0 = node_of(d, ix, iy, iz);
                for (int a = 0; a < 3; ++a) {
                    if (i3[a] + 1 < d[a]) edges.push_back({{n0, n0 + stride[a], 0}, 2});
                    if (i3[a] + 2 < d[a]) triples.push_back({{n0, n0 + stride[a], n0 + 2 * stride[a]}, 3});
                }
            }
}

// "" or why a cell's sums cannot be sums of g g', g r0, r0^2 over n points: the count, and the 25 x 25 Gram matrix [A b; b' S_rr]
// positive semi-definite to rounding (its LDL' after a shift of (1e-10 + 8 n 2^-52) trace keeps positive pivots)
inline std::string check_cell(const double* s, int cell) {
    char msg[160];
    const double n = s[325];
    if (!(n >= 0) || n != floor(n)) { snprintf(msg, sizeof msg, "cell %d: count %g is not a non-negative integer", cell, n); return msg; }
    double G[25][25];
    for (int a = 0; a < 24; ++a)
        for (int b = a; b < 24; ++b) G[a][b] = G[b][a] = s[tri(a, b)];
    for (int a = 0; a < 24; ++a) G[a][24] = G[24][a] = s[300 + a];
    G[24][24] = s[324];
    double trace = 0, big = 0;
    for (int a = 0; a < 25; ++a) {
        if (G[a][a] < 0) { snprintf(msg, sizeof msg, "cell %d: negative diagonal %g at %d", cell, G[a][a], a); return msg; }
        trace += G[a][a];
        for (int b = 0; b < 25; ++b) big = fmax(big, fabs(G[a][b]));
    }
    if (n == 0 && big != 0) { snprintf(msg, sizeof msg, "cell %d: no correspondence but non-zero sums", cell); return msg; }
    if (trace == 0) {
        if (big != 0) { snprintf(msg, sizeof msg, "cell %d: zero diagonal but non-zero entries", cell); return msg; }
        return "";
    }
    const double shift = (1e-10 + 8.0 * n * 2.220446049250313e-16) * trace;
    for (int a = 0; a < 25; ++a) G[a][a] += shift;
    for (int j = 0; j < 25; ++j) {                       // LDL' in place, no pivoting
        if (!(G[j][j] > 0)) { snprintf(msg, sizeof msg, "cell %d: the block of sums is not symmetric positive semi-definite (pivot %d: %g)", cell, j, G[j][j]); return msg; }
        for (int i = j + 1; i < 25; ++i) {
            const double l = G[i][j] / G[j][j];
            for (int k = j + 1; k <= i; ++k) G[i][k] -= l * G[k][j];
        }
    }
    return "";
}

// E(U) from the sums, term by term (not through H): the data term goes to *data
inline double energy(const int32_t d[3], const double* sums, double wT, double wE, double w0, const std::vector<Stencil>& triples,
                     const std::vector<Stencil>& edges, const double* U, double* data) {
    double Ed = 0;
    const int nc = n_cells(d);
    for (int c = 0; c < nc; ++c) {
        const double* s = sums + (size_t)c * CELL_LEN;
        if (s[325] == 0) continue;
        int nd[8];
        cell_nodes(d, c, nd);
        double u[24];
        for (int k = 0; k < 8; ++k)
            for (int a = 0; a < 3; ++a) u[3 * k + a] = U[3 * nd[k] + a];
        double q = 0, l = 0;
        for (int a = 0; a < 24; ++a) {
            l += s[300 + a] * u[a];
            q += s[tri(a, a)] * u[a] * u[a];
            for (int b = a + 1; b < 24; ++b) q += 2.0 * s[tri(a, b)] * u[a] * u[b];
        }
        Ed += s[324] + 2.0 * l + q;
    }
    double Et = 0, Ee = 0, E0 = 0;
    for (const Stencil& t : triples)
        for (int a = 0; a < 3; ++a) { const double v = U[3 * t.node[0] + a] - 2.0 * U[3 * t.node[1] + a] + U[3 * t.node[2] + a]; Et += v * v; }
    for (const Stencil& e : edges)
        for (int a = 0; a < 3; ++a) { const double v = U[3 * e.node[0] + a] - U[3 * e.node[1] + a]; Ee += v * v; }
    const int M = n_nodes(d);
    for (int i = 0; i < 3 * M; ++i) E0 += U[i] * U[i];
    if (data) *data = Ed;
    return Ed + wT * Et + wE * Ee + w0 * E0;
}

// U: on entry the displacements the sums were taken at (only E_before reads them), on exit the minimiser of E.  "" or the refusal.
inline std::string solve(const int32_t dims[3], const double* sums, double lam, double lam0, double* U, Report* rep) {
    char msg[200];
    if (!dims || !sums || !U) return "NULL argument";
    if (!dims_ok(dims)) { snprintf(msg, sizeof msg, "lattice dimensions (%d, %d, %d) outside [%d, %d]", dims[0], dims[1], dims[2], MIN_DIM, MAX_DIM); return msg; }
    if (!(lam == lam) || !(lam0 == lam0) || isinf(lam) || isinf(lam0)) return "non-finite regularisation weight";
    if (lam < 0 || lam0 < 0) { snprintf(msg, sizeof msg, "negative regularisation weight (lam %g, lam0 %g)", lam, lam0); return msg; }
    const int M = n_nodes(dims), nc = n_cells(dims), N = 3 * M;
    for (size_t i = 0; i < (size_t)nc * CELL_LEN; ++i)
        if (!isfinite(sums[i])) { snprintf(msg, sizeof msg, "non-finite sum (cell %zu, slot %zu)", i / CELL_LEN, i % CELL_LEN); return msg; }
    for (int i = 0; i < N; ++i)
        if (!isfinite(U[i])) { snprintf(msg, sizeof msg, "non-finite displacement (node %d)", i / 3); return msg; }
    double nC = 0;
    for (int c = 0; c < nc; ++c) {
        const std::string e = check_cell(sums + (size_t)c * CELL_LEN, c);
        if (!e.empty()) return e;
        nC += sums[(size_t)c * CELL_LEN + 325];
    }
    std::vector<Stencil> triples, edges;
    stencils(dims, triples, edges);
    const double wT = triples.empty() ? 0.0 : lam * nC / (double)triples.size();
    const double wE = edges.empty() ? 0.0 : 0.01 * lam * nC / (double)edges.size();
    const double w0 = lam0 * nC / (double)M;
    Report r;
    r.n_corr = (int64_t)nC;
    r.n_unknowns = N;
    r.E_before = energy(dims, sums, wT, wE, w0, triples, edges, U, &r.E_data_before);
    if (nC == 0) {                                   // nothing to fit and every weight is 0: the field stays flat
        for (int i = 0; i < N; ++i) U[i] = 0.0;
        r.E_after = r.E_data_after = 0.0;
        if (rep) *rep = r;
        return "";
    }
    int hb = 3 * (dims[1] * dims[2] + dims[2] + 1) + 2;                       // the cell's far corner
    if (dims[0] > 2) hb = 3 * 2 * dims[1] * dims[2] + 2;                        // the second difference along x
    if (hb > N - 1) hb = N - 1;
    r.half_band = hb;
    const size_t W = (size_t)hb + 1;
    std::vector<double> B((size_t)N * W, 0.0), rhs((size_t)N, 0.0);           // row i holds H(i, i - hb .. i), the diagonal last
    auto at = [&](int i, int j) -> double& { return B[(size_t)i * W + (size_t)(hb + j - i)]; };      // j <= i
    for (int c = 0; c < nc; ++c) {
        const double* s = sums + (size_t)c * CELL_LEN;
        if (s[325] == 0) continue;
        int nd[8];
        cell_nodes(dims, c, nd);
        for (int a = 0; a < 24; ++a) {
            const int i = 3 * nd[a / 3] + a % 3;
            rhs[i] -= s[300 + a];
            for (int b = a; b < 24; ++b) {
                const int j = 3 * nd[b / 3] + b % 3;
                if (i >= j) at(i, j) += s[tri(a, b)]; else at(j, i) += s[tri(a, b)];
            }
        }
    }
    auto add_stencil = [&](const Stencil& t, const double* coef, double w) {
        for (int p = 0; p < t.len; ++p)
            for (int q = 0; q <= p; ++q)                 // node[p] > node[q] for q < p
                for (int a = 0; a < 3; ++a) at(3 * t.node[p] + a, 3 * t.node[q] + a) += w * coef[p] * coef[q];
    };
    const double c3[3] = {1.0, -2.0, 1.0}, c2[2] = {1.0, -1.0};
    if (wT > 0) for (const Stencil& t : triples) add_stencil(t, c3, wT);
    if (wE > 0) for (const Stencil& e : edges) add_stencil(e, c2, wE);
    for (int i = 0; i < N; ++i) at(i, i) += w0;
    // banded Cholesky H = L L', L over B
    r.pivot_min = INFINITY; r.pivot_max = 0;
    for (int j = 0; j < N; ++j) {
        const double* rj = &B[(size_t)j * W];
        const int k0 = j - hb > 0 ? j - hb : 0;
        double dj = rj[hb];
        for (int k = k0; k < j; ++k) { const double v = rj[hb + k - j]; dj -= v * v; }
        if (!(dj > 0)) {
            snprintf(msg, sizeof msg, "the system is not positive definite (pivot %d of %d: %g): with lam0 = 0 empty cells leave nodes undetermined", j, N, dj);
            return msg;
        }
        r.pivot_min = fmin(r.pivot_min, dj); r.pivot_max = fmax(r.pivot_max, dj);
        const double ljj = sqrt(dj);
        B[(size_t)j * W + hb] = ljj;
        const int i1 = j + hb < N - 1 ? j + hb : N - 1;
        for (int i = j + 1; i <= i1; ++i) {
            double* ri = &B[(size_t)i * W];
            const int ka = i - hb > k0 ? i - hb : k0;
            double v = ri[hb + j - i];
            for (int k = ka; k < j; ++k) v -= ri[hb + k - i] * rj[hb + k - j];
            ri[hb + j - i] = v / ljj;
        }
    }
    for (int i = 0; i < N; ++i) {                        // L y = rhs
        const double* ri = &B[(size_t)i * W];
        double v = rhs[i];
        for (int k = i - hb > 0 ? i - hb : 0; k < i; ++k) v -= ri[hb + k - i] * rhs[k];
        rhs[i] = v / ri[hb];
    }
    for (int i = N - 1; i >= 0; --i) {                   // L' x = y
        double v = rhs[i];
        const int i1 = i + hb < N - 1 ? i + hb : N - 1;
        for (int k = i + 1; k <= i1; ++k) v -= B[(size_t)k * W + (size_t)(hb + i - k)] * rhs[k];
        rhs[i] = v / B[(size_t)i * W + hb];
    }
    for (int i = 0; i < N; ++i) U[i] = rhs[i];
    r.E_after = energy(dims, sums, wT, wE, w0, triples, edges, U, &r.E_data_after);
    if (rep) *rep = r;
    return "";
}

}  // namespace warp
}  // namespace gsr
