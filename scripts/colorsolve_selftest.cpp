// Stand-alone host program over csrc/gsr_colorsolve.h for a sanitizer run (the header has no HIP include):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/colorsolve_selftest.cpp -o colorsolve_selftest
//     ./colorsolve_selftest
//
// Every scene i has a ground-truth transform G_i (the reference's is [I|0]); scene i shows a surface of true colour y as
// x = G_i^-1 (y): the transforms that bring the scenes into agreement with the reference are P_i = G_i.  Exact sums of random pairs:
// Case 1: two scenes, every mode, the known transform comes back within 1e-9.
// Case 2: a chain 0-1-2-3 with the loop closure 3-0, a fifth scene without an edge and a sixth behind an edge of 5 pairs: the four
//         come back jointly, the two others are held, flagged, and keep their bits; the reference's doubles are never written.
// Case 3: the refusals (bad index, source == target, NaN, unknown mode, negative prior, singular with prior = 0).
// Exit status 0 and "ok" when all hold.
#include "../gaussiansplattingregistration_amd/csrc/gsr_colorsolve.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace gsr::colorsolve;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                     // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0;
}

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_failed; } } while (0)

static void identity(double* P) { for (int k = 0; k < 12; ++k) P[k] = k % 5 == 0 ? 1.0 : 0.0; }
// the ground truth of a mode: gains in [0.7, 1.3], off-diagonals and offsets within 0.1 (affine only)
static void random_truth(int mode, double* G) {
    identity(G);
    if (mode == GAIN) { const double g = 0.7 + 0.6 * uniform(); G[0] = G[5] = G[10] = g; }
    else if (mode == CHANNEL_GAIN) for (int c = 0; c < 3; ++c) G[5 * c] = 0.7 + 0.6 * uniform();
    else for (int k = 0; k < 12; ++k) G[k] += 0.2 * uniform() - 0.1;
}
// x with G [x; 1] = y (3 x 3 solve by Cramer's rule)
static void inverse_apply(const double* G, const double* y, double* x) {
    const double a = G[0], b = G[1], c = G[2], d = G[4], e = G[5], f = G[6], g = G[8], h = G[9], i = G[10];
    const double r[3] = {y[0] - G[3], y[1] - G[7], y[2] - G[11]};
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    x[0] = (r[0] * (e * i - f * h) - b * (r[1] * i - f * r[2]) + c * (r[1] * h - e * r[2])) / det;
    x[1] = (a * (r[1] * i - f * r[2]) - r[0] * (d * i - f * g) + c * (d * r[2] - r[1] * g)) / det;
    x[2] = (a * (e * r[2] - r[1] * h) - b * (d * r[2] - r[1] * g) + r[0] * (d * h - e * g)) / det;
}
static Edge make_edge(int s, int t, const double* Gs, const double* Gt, int n, bool grey = false) {
    Edge e;
    e.s = s; e.t = t;
    for (int k = 0; k < SUMS_LEN; ++k) e.sums[k] = 0.0;
    for (int p = 0; p < n; ++p) {
        double y[3] = {uniform(), uniform(), uniform()};
        if (grey) y[1] = y[2] = y[0];
        double a[4], b[4];
        inverse_apply(Gs, y, a);
        inverse_apply(Gt, y, b);
        a[3] = b[3] = 1.0;
        const double w = 0.2 + 0.8 * uniform();
        e.sums[0] += 1.0;
        e.sums[1] += w;
        int k = 3;
        for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) e.sums[k++] += w * a[i] * a[j];
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) e.sums[k++] += w * a[i] * b[j];
        for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) e.sums[k++] += w * b[i] * b[j];
    }
    return e;
}
static double max_diff(const double* A, const double* B) {
    double m = 0;
    for (int k = 0; k < 12; ++k) m = fmax(m, fabs(A[k] - B[k]));
    return m;
}

int main() {
    const char* names[3] = {"gain", "channel_gain", "affine"};
    for (int mode = 0; mode < 3; ++mode) {
        // ---- case 1
        double G[24], P[24];
        identity(G);
        random_truth(mode, G + 12);
        identity(P); identity(P + 12);
        std::vector<Edge> E{make_edge(1, 0, G + 12, G, 500)};
        Result r;
        int32_t held[2] = {-1, -1};
        std::string err = solve(2, P, E, mode, 0.0, 100, 0, held, &r);
        CHECK(err.empty(), "%s: %s", names[mode], err.c_str());
        CHECK(max_diff(P + 12, G + 12) < 1e-9, "%s: two scenes, error %g", names[mode], max_diff(P + 12, G + 12));
        CHECK(held[0] == 1 && held[1] == 0 && r.n_free == 1 && r.n_unknowns == mode_dim(mode), "%s: held / free", names[mode]);
        CHECK(r.E_final <= r.E_initial && r.E_final < 1e-12 * (1 + r.E_initial), "%s: objective %g -> %g", names[mode], r.E_initial, r.E_final);
        CHECK(r.pivot_min > 0 && r.pivot_max >= r.pivot_min, "%s: pivots %g %g", names[mode], r.pivot_min, r.pivot_max);
        // ---- case 2
        const int N = 6;
        std::vector<double> Gt(12 * N), Pn(12 * N);
        for (int i = 0; i < N; ++i) { identity(&Pn[12 * i]); random_truth(mode, &Gt[12 * i]); }
        const int ref = 1;
        identity(&Gt[12 * ref]);
        // node 4 has no edge and starts anywhere; node 5's weak edge stays in the objective, so it starts at its truth
        for (int k = 0; k < 12; ++k) { Pn[12 * 4 + k] = 0.5 * Gt[12 * 4 + k]; Pn[12 * 5 + k] = Gt[12 * 5 + k]; }
        std::vector<Edge> E2{make_edge(0, 1, &Gt[0], &Gt[12], 400), make_edge(1, 2, &Gt[12], &Gt[24], 400), make_edge(2, 3, &Gt[24], &Gt[36], 400),
                             make_edge(3, 0, &Gt[36], &Gt[0], 400), make_edge(5, 2, &Gt[60], &Gt[24], 5)};
        std::vector<double> before(Pn);
        int32_t held2[N];
        err = solve(N, Pn.data(), E2, mode, 1e-9, 100, ref, held2, &r);
        CHECK(err.empty(), "%s: %s", names[mode], err.c_str());
        for (int i = 0; i < 4; ++i)
            CHECK(max_diff(&Pn[12 * i], &Gt[12 * i]) < 1e-6, "%s: graph, node %d error %g", names[mode], i, max_diff(&Pn[12 * i], &Gt[12 * i]));
        for (int i : {ref, 4, 5}) CHECK(memcmp(&Pn[12 * i], &before[12 * i], 96) == 0, "%s: held node %d was written", names[mode], i);
        const int32_t want[N] = {0, 1, 0, 0, 1, 1};
        CHECK(memcmp(held2, want, sizeof want) == 0, "%s: held flags", names[mode]);
        CHECK(r.n_free == 3, "%s: %d free nodes", names[mode], r.n_free);
    }
    // ---- case 3
    {
        double G[24], P[24];
        identity(G); random_truth(AFFINE, G + 12); identity(P); identity(P + 12);
        std::vector<Edge> E{make_edge(1, 0, G + 12, G, 300)};
        auto refused = [&](const char* what, const std::string& err) { CHECK(!err.empty(), "%s was accepted", what); };
        std::vector<Edge> B = E;
        B[0].t = 2;
        refused("index out of range", solve(2, P, B, AFFINE, 1e-4, 100, 0, nullptr, nullptr));
        B = E; B[0].t = 1;
        refused("source == target", solve(2, P, B, AFFINE, 1e-4, 100, 0, nullptr, nullptr));
        B = E; B[0].sums[7] = NAN;
        refused("NaN sum", solve(2, P, B, AFFINE, 1e-4, 100, 0, nullptr, nullptr));
        P[13] = INFINITY;
        refused("non-finite P", solve(2, P, E, AFFINE, 1e-4, 100, 0, nullptr, nullptr));
        identity(P + 12);
        refused("unknown mode", solve(2, P, E, 7, 1e-4, 100, 0, nullptr, nullptr));
        refused("negative prior", solve(2, P, E, AFFINE, -1.0, 100, 0, nullptr, nullptr));
        refused("NaN prior", solve(2, P, E, AFFINE, NAN, 100, 0, nullptr, nullptr));
        refused("reference out of range", solve(2, P, E, AFFINE, 1e-4, 100, 2, nullptr, nullptr));
        std::vector<Edge> Gy{make_edge(1, 0, G, G, 300, true)};
        const std::string err = solve(2, P, Gy, AFFINE, 0.0, 100, 0, nullptr, nullptr);
        CHECK(err.find("raise prior") != std::string::npos, "grey colours, prior 0: '%s'", err.c_str());
        CHECK(solve(2, P, Gy, AFFINE, 1e-4, 100, 0, nullptr, nullptr).empty(), "grey colours with a prior were refused");
        CHECK(solve(2, P, std::vector<Edge>(), AFFINE, 1e-4, 100, 0, nullptr, nullptr).empty(), "a graph without edges was refused");
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok\n");
    return 0;
}
