// Stand-alone host program over csrc/gsr_posegraph.h for a sanitizer run (the header has no HIP include):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/posegraph_selftest.cpp -o posegraph_selftest
//     ./posegraph_selftest
//
// Case 1: a consistent graph (exact edges) from a start 0.05 rad / 0.05 units off returns to ground truth within 1e-8.
// Case 3: five odometry edges (1e-3 noise), four loop closures (2e-4 noise) and one false loop closure (30 degrees, 0.6 units off):
// exactly the false edge is pruned, the true loops keep l >= 0.9.  Also the refusals (unreachable node, bad index, bad matrix).
// Exit status 0 and "ok" when all hold.
#include "../gaussiansplattingregistration_amd/csrc/gsr_posegraph.h"

#include <stdio.h>
#include <stdlib.h>

using namespace gsr::posegraph;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                     // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0;
}
static double normal() { return sqrt(-2.0 * log(1.0 - uniform())) * cos(6.283185307179586 * uniform()); }

static void make_pose(const double* w, const double* t, double* X) {
    double R[9];
    so3_exp(w, R);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) X[4 * i + j] = R[3 * i + j]; X[4 * i + 3] = t[i]; }
    X[12] = X[13] = X[14] = 0; X[15] = 1;
}
static void random_pose(double rot, double trans, double* X) {
    const double w[3] = {rot * normal(), rot * normal(), rot * normal()}, t[3] = {trans * normal(), trans * normal(), trans * normal()};
    make_pose(w, t, X);
}

static Edge make_edge(const std::vector<double>& gt, int s, int t, double noise, bool uncertain, const double* off) {
    Edge e;
    e.s = s; e.t = t; e.uncertain = uncertain;
    double Xti[16], N[16];
    rigid_inv(&gt[16 * t], Xti);
    rigid_mul(Xti, &gt[16 * s], e.T);
    if (noise > 0) { random_pose(noise, noise, N); rigid_mul(N, e.T, e.T); }
    if (off) rigid_mul(off, e.T, e.T);
    for (int i = 0; i < 36; ++i) e.info[i] = 0;
    for (int k = 0; k < 2000; ++k) {         // sum G^T G, G = [-[q]x | I], q = a scene point in the target's frame
        const double p[3] = {2 * (uniform() - 0.5), 2 * (uniform() - 0.5), 2 * (uniform() - 0.5)};
        double q[3], S[9], G[18];
        for (int i = 0; i < 3; ++i) q[i] = Xti[4 * i] * p[0] + Xti[4 * i + 1] * p[1] + Xti[4 * i + 2] * p[2] + Xti[4 * i + 3];
        skew(q, S);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { G[6 * i + j] = -S[3 * i + j]; G[6 * i + 3 + j] = i == j; }
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) for (int i = 0; i < 3; ++i) e.info[6 * a + b] += G[6 * i + a] * G[6 * i + b];
    }
    return e;
}

static double pose_error(const std::vector<double>& X, const std::vector<double>& gt) {
    double worst = 0;
    for (size_t i = 0; i < X.size() / 16; ++i) {
        double s = 0;
        for (int k = 0; k < 16; ++k) s += (X[16 * i + k] - gt[16 * i + k]) * (X[16 * i + k] - gt[16 * i + k]);
        worst = fmax(worst, sqrt(s));
    }
    return worst;
}

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }    \
    } while (0)

int main() {
    const int N = 6;
    std::vector<double> gt(16 * N);
    for (int k = 0; k < 16; ++k) gt[k] = (k % 5 == 0);
    for (int i = 1; i < N; ++i) random_pose(0.4, 1.0, &gt[16 * i]);
    const int loops[4][2] = {{0, 2}, {1, 4}, {0, 5}, {2, 5}};
    Option tight;
    tight.max_correspondence_distance = 0.05;
    tight.max_iteration = 1000;
    tight.min_relative_increment = tight.min_relative_residual_increment = 1e-12;
    tight.min_right_term = tight.min_residual = 0;

    {   // case 1
        std::vector<Edge> E;
        for (int i = 0; i + 1 < N; ++i) E.push_back(make_edge(gt, i, i + 1, 0, false, nullptr));
        for (auto& l : loops) E.push_back(make_edge(gt, l[0], l[1], 0, true, nullptr));
        std::vector<double> X(gt);
        for (int i = 1; i < N; ++i) { double P[16]; random_pose(0.03, 0.03, P); rigid_mul(P, &gt[16 * i], &X[16 * i]); }
        const double e0 = pose_error(X, gt);
        std::vector<double> l(E.size());
        std::vector<int32_t> pr(E.size());
        Result r;
        const std::string err = optimize(N, X.data(), E, tight, l.data(), pr.data(), &r);
        CHECK(err.empty());
        const double e1 = pose_error(X, gt);
        printf("case 1: error %.3e -> %.3e, E %.3e -> %.3e, iterations %d + %d\n", e0, e1, r.E_initial, r.E_final, r.iterations[0], r.iterations[1]);
        CHECK(e0 > 0.03 && e1 <= 1e-8 && r.n_pruned == 0);
    }
    {   // case 3
        std::vector<Edge> E;
        for (int i = 0; i + 1 < N; ++i) E.push_back(make_edge(gt, i, i + 1, 1e-3, false, nullptr));
        for (auto& l : loops) E.push_back(make_edge(gt, l[0], l[1], 2e-4, true, nullptr));
        double off[16];
        const double w[3] = {0.3, -0.35, 0.25}, t[3] = {0.4, -0.3, 0.33};
        make_pose(w, t, off);
        E.push_back(make_edge(gt, 1, 3, 2e-4, true, off));
        std::vector<double> X(16 * N);
        for (int k = 0; k < 16; ++k) X[k] = gt[k];
        for (int i = 0; i + 1 < N; ++i) { double Ti[16]; rigid_inv(E[i].T, Ti); rigid_mul(&X[16 * i], Ti, &X[16 * (i + 1)]); }     // chained odometry
        const double e0 = pose_error(X, gt);
        std::vector<double> l(E.size());
        std::vector<int32_t> pr(E.size());
        Result r;
        const std::string err = optimize(N, X.data(), E, tight, l.data(), pr.data(), &r);
        CHECK(err.empty());
        const double e1 = pose_error(X, gt);
        printf("case 3: error %.3e -> %.3e, mu %.4f, pruned %d, l =", e0, e1, r.mu, r.n_pruned);
        for (double v : l) printf(" %.5f", v);
        printf("\n");
        CHECK(r.n_pruned == 1 && pr.back() == 1 && l.back() < 0.25);
        for (size_t k = 0; k + 1 < E.size(); ++k) CHECK(pr[k] == 0 && l[k] >= 0.9);
        CHECK(e1 < e0);
        // refusals
        std::vector<Edge> few(E.begin(), E.begin() + 2);
        CHECK(optimize(N, X.data(), few, tight, nullptr, nullptr, nullptr).find("cannot be reached") != std::string::npos);
        std::vector<Edge> bad(E);
        bad[3].t = N;
        CHECK(optimize(N, X.data(), bad, tight, nullptr, nullptr, nullptr).find("out of range") != std::string::npos);
        bad = E;
        bad[2].info[1] += 1.0;
        CHECK(optimize(N, X.data(), bad, tight, nullptr, nullptr, nullptr).find("not symmetric") != std::string::npos);
        bad = E;
        bad[2].info[0] = -1.0;
        CHECK(optimize(N, X.data(), bad, tight, nullptr, nullptr, nullptr).find("semi-definite") != std::string::npos);
    }
    printf("ok\n");
    return 0;
}
