// warp_selftest.cpp -- csrc/gsr_warp.h (the host solver of non-rigid refinement) as a stand-alone program: every
// refusal, the empty problem, and one small solve checked against its own normal equations.  Built with -fsanitize=address,undefined
// by tests/test_warp_cpu.py; nothing of the library is linked.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/warp_selftest.cpp -o warp_selftest && ./warp_selftest
#include <stdio.h>
#include <stdlib.h>

#include "../gaussiansplattingregistration_amd/csrc/gsr_warp.h"

using namespace gsr::warp;

static int failures = 0;
#define EXPECT(cond, what)                                                   \
    do {                                                                     \
        if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); ++failures; } \
    } while (0)

static double urand(unsigned* s) { *s = *s * 1664525u + 1013904223u; return (double)(*s >> 8) / 16777216.0; }

// sums of `npts` random correspondences in cells picked at random (only_cell >= 0: all in that cell)
static std::vector<double> random_sums(const int32_t d[3], int npts, int only_cell, unsigned seed) {
    std::vector<double> sums((size_t)n_cells(d) * CELL_LEN, 0.0);
    for (int i = 0; i < npts; ++i) {
        const int cell = only_cell >= 0 ? only_cell : (int)(urand(&seed) * n_cells(d)) % n_cells(d);
        double f[3], n[3], nn = 0;
        for (int a = 0; a < 3; ++a) { f[a] = urand(&seed); n[a] = urand(&seed) - 0.5; nn += n[a] * n[a]; }
        for (int a = 0; a < 3; ++a) n[a] /= sqrt(nn);
        const double r0 = 0.1 * (urand(&seed) - 0.5);
        double g[24];
        for (int k = 0; k < 8; ++k) {
            const double w = ((k & 4) ? f[0] : 1 - f[0]) * ((k & 2) ? f[1] : 1 - f[1]) * ((k & 1) ? f[2] : 1 - f[2]);
            for (int a = 0; a < 3; ++a) g[3 * k + a] = w * n[a];
        }
        double* s = &sums[(size_t)cell * CELL_LEN];
        for (int a = 0; a < 24; ++a) {
            for (int b = a; b < 24; ++b) s[tri(a, b)] += g[a] * g[b];
            s[300 + a] += g[a] * r0;
        }
        s[324] += r0 * r0;
        s[325] += 1.0;
    }
    return sums;
}

int main() {
    const int32_t d[3] = {2, 3, 5};
    const int M = n_nodes(d);
    std::vector<double> sums = random_sums(d, 400, -1, 7u), U((size_t)3 * M, 0.0);
    Report r;
    std::string e;

    // refusals
    { const int32_t bad[3] = {1, 3, 3}; e = solve(bad, sums.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "dimension 1 accepted"); }
    { const int32_t bad[3] = {3, 18, 3}; std::vector<double> s2((size_t)2 * 17 * 2 * CELL_LEN, 0.0), u2((size_t)3 * 3 * 18 * 3, 0.0);
      e = solve(bad, s2.data(), 0.01, 1e-6, u2.data(), &r); EXPECT(!e.empty(), "dimension 18 accepted"); }
    e = solve(d, sums.data(), -0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "negative lam accepted");
    e = solve(d, sums.data(), 0.01, -1e-6, U.data(), &r); EXPECT(!e.empty(), "negative lam0 accepted");
    e = solve(d, sums.data(), NAN, 1e-6, U.data(), &r); EXPECT(!e.empty(), "NaN lam accepted");
    { std::vector<double> s2 = sums; s2[5] = NAN; e = solve(d, s2.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "NaN sum accepted"); }
    { std::vector<double> s2 = sums; s2[CELL_LEN + 300] = INFINITY; e = solve(d, s2.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "inf sum accepted"); }
    { std::vector<double> u2 = U; u2[4] = NAN; e = solve(d, sums.data(), 0.01, 1e-6, u2.data(), &r); EXPECT(!e.empty(), "NaN U accepted"); }
    { std::vector<double> s2 = sums; s2[tri(3, 3)] = -s2[tri(3, 3)] - 1.0; e = solve(d, s2.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "negative diagonal accepted"); }
    { std::vector<double> s2 = sums; s2[tri(0, 1)] = 10.0 * (s2[tri(0, 0)] + s2[tri(1, 1)] + 1.0); e = solve(d, s2.data(), 0.01, 1e-6, U.data(), &r);
      EXPECT(!e.empty(), "indefinite block accepted"); }
    { std::vector<double> s2 = sums; s2[325] = 2.5; e = solve(d, s2.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "fractional count accepted"); }
    { std::vector<double> s2 = sums; s2[325] = -1.0; e = solve(d, s2.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "negative count accepted"); }
    e = solve(nullptr, sums.data(), 0.01, 1e-6, U.data(), &r); EXPECT(!e.empty(), "NULL dims accepted");
    {   // lam0 = 0 and lam = 0 with data in one cell of a 5^3 lattice: nodes without data are undetermined
        const int32_t d5[3] = {5, 5, 5};
        std::vector<double> s5 = random_sums(d5, 50, 10, 3u), u5((size_t)3 * 125, 0.0);
        e = solve(d5, s5.data(), 0.0, 0.0, u5.data(), &r); EXPECT(!e.empty(), "singular system accepted");
        e = solve(d5, s5.data(), 0.01, 1e-6, u5.data(), &r); EXPECT(e.empty(), "regularised one-cell system refused");
        EXPECT(r.E_after <= r.E_before, "the minimiser raised E (one cell)");
    }

    // no correspondence: U = 0
    {
        std::vector<double> s0((size_t)n_cells(d) * CELL_LEN, 0.0), u0((size_t)3 * M, 0.25);
        e = solve(d, s0.data(), 0.01, 1e-6, u0.data(), &r);
        EXPECT(e.empty(), "empty problem refused");
        bool zero = true;
        for (double v : u0) zero = zero && v == 0.0;
        EXPECT(zero && r.n_corr == 0 && r.E_after == 0.0, "empty problem: U != 0");
    }

    // one solve: the gradient of E vanishes at the result (central differences of energy()), and E fell
    e = solve(d, sums.data(), 0.01, 1e-6, U.data(), &r);
    EXPECT(e.empty(), "valid problem refused");
    EXPECT(r.n_corr == 400 && r.n_unknowns == 3 * M, "report");
    EXPECT(r.E_after < r.E_before, "E did not fall");
    {
        std::vector<Stencil> triples, edges;
        stencils(d, triples, edges);
        const double nC = 400.0, wT = 0.01 * nC / triples.size(), wE = 1e-4 * nC / edges.size(), w0 = 1e-6 * nC / M;
        double worst = 0;
        for (int i = 0; i < 3 * M; ++i) {
            const double keep = U[i], h = 1e-4;
            U[i] = keep + h; const double ep = energy(d, sums.data(), wT, wE, w0, triples, edges, U.data(), nullptr);
            U[i] = keep - h; const double em = energy(d, sums.data(), wT, wE, w0, triples, edges, U.data(), nullptr);
            U[i] = keep;
            worst = fmax(worst, fabs(ep - em) / (2 * h));
        }
        printf("2x3x5: E %.6g -> %.6g, half band %d, pivots [%.3g, %.3g], max |dE/dU| at the solution %.3g\n", r.E_before, r.E_after, r.half_band, r.pivot_min,
               r.pivot_max, worst);
        EXPECT(worst < 1e-9 * (1.0 + r.E_before), "the gradient does not vanish at the solution");
    }
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
