// orient_selftest.cpp -- the round logic of the normal orientation (csrc/gsr_orient.h) run serially on the host, against a Kruskal
// forest and a depth-first propagation written here, as a stand-alone program for the host sanitizers.  No HIP, no device:
//
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/orient_selftest.cpp -o orient_selftest
//     ./orient_selftest
//
// The graphs: random lists with tied weights, duplicates, self entries, entries outside [0, n), empty rows, dead (NaN) normals,
// and chains whose single round hooks n - 1 roots one behind the other.  A cycle or an index out of bounds in the hooking or the
// parent walks shows here, before anything runs on a GPU.  Exit status 0 and "ok" when every case agrees.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <tuple>
#include <vector>

#include "../gaussiansplattingregistration_amd/csrc/gsr_orient.h"

using namespace gsr;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct Case {
    int64_t n;
    int32_t stride;
    std::vector<float> xyz;
    std::vector<double> nrm;
    std::vector<int32_t> nbr, count;
    bool vote;
    double c[3];
};
struct Result {
    std::vector<uint8_t> flip;
    std::vector<int32_t> component;
    int64_t n_components = 0, n_flipped = 0, n_not_live = 0;
    int rounds = 0;
    bool ok = true;
};

// ---- the steps of gsr_orient.h in the order csrc/orient.hip launches them, a loop where the device has a kernel
static Result run_steps(const Case& in) {
    const int64_t n = in.n;
    Result R;
    std::vector<double> nrm = in.nrm;
    std::vector<uint8_t> live(n);
    std::vector<uint32_t> par(n), par2(n);
    std::vector<int32_t> deg(n + 1, 0), off(n + 1, 0), cursor(n), label(n, 0x7f7f7f7f), toward(n, 0), away(n, 0);
    R.component.assign(n, -1);
    for (int64_t v = 0; v < n; ++v) orient_init_vertex(v, nrm.data(), live.data(), par.data(), deg.data(), cursor.data());
    for (int64_t v = 0; v < n; ++v) orient_count_vertex(v, n, in.nbr.data(), in.stride, in.count.data(), live.data(), deg.data());
    for (int64_t v = 0; v < n; ++v) off[v + 1] = off[v] + deg[v];
    std::vector<int32_t> adj(off[n]);
    std::vector<uint64_t> key(off[n]);
    for (int64_t v = 0; v < n; ++v)
        orient_fill_vertex(v, n, in.nbr.data(), in.stride, in.count.data(), live.data(), nrm.data(), off.data(), cursor.data(), adj.data(), key.data());
    for (int64_t v = 0; v < n; ++v) EXPECT(cursor[v] == deg[v]);
    const int launches = orient_jump_launches(n);
    std::vector<uint64_t> minw(n), minlohi(n);
    for (;; ++R.rounds) {
        if (R.rounds == ORIENT_MAX_ROUNDS) { R.ok = false; return R; }
        std::fill(minw.begin(), minw.end(), ORIENT_NONE);
        std::fill(minlohi.begin(), minlohi.end(), ORIENT_NONE);
        for (int64_t v = 0; v < n; ++v) orient_min_weight_vertex(v, par.data(), off.data(), adj.data(), key.data(), minw.data());
        for (int64_t v = 0; v < n; ++v) orient_min_edge_vertex(v, par.data(), off.data(), adj.data(), key.data(), minw.data(), minlohi.data());
        int64_t hooks = 0;
        for (int64_t v = 0; v < n; ++v) hooks += orient_hook_vertex(v, par.data(), par2.data(), nrm.data(), minw.data(), minlohi.data()) ? 1 : 0;
        if (!hooks) break;
        // the device runs the walks of one launch in any order and sees any mixture of old and new words: descending order is
        // the slowest serial one (every walk reads words no walk of this launch has shortened yet, as a synchronous step would)
        for (int l = 0; l < launches; ++l)
            for (int64_t v = n - 1; v >= 0; --v) orient_jump_vertex(v, par2.data());
        for (int64_t v = 0; v < n; ++v)
            if (!orient_is_flat(v, par2.data())) { R.ok = false; return R; }
        par.swap(par2);
    }
    for (int64_t v = 0; v < n; ++v) ORIENT_MIN_I32(&label[par[v] & ORIENT_PARENT], v);
    if (in.vote)
        for (int64_t v = 0; v < n; ++v) {
            const int t = orient_vote_vertex(v, par.data(), label.data(), live.data(), in.xyz.data(), nrm.data(), in.c[0], in.c[1], in.c[2]);
            if (t > 0) ++toward[par[v] & ORIENT_PARENT];
            if (t < 0) ++away[par[v] & ORIENT_PARENT];
        }
    R.flip.assign(n, 0);
    for (int64_t v = 0; v < n; ++v) {
        const int what = orient_flip_vertex(v, par.data(), label.data(), live.data(), toward.data(), away.data(), in.vote, nrm.data(), R.component.data());
        R.flip[v] = (what & ORIENT_IS_FLIPPED) ? 1 : 0;
        R.n_flipped += R.flip[v];
        R.n_components += (what & ORIENT_IS_ROOT) ? 1 : 0;
        R.n_not_live += (what & ORIENT_IS_NOT_LIVE) ? 1 : 0;
        for (int k = 0; k < 3; ++k) {                                 // the input or its exact negation, dead rows untouched
            const double a = in.nrm[v * 3 + k], b = nrm[v * 3 + k];
            const double want = R.flip[v] ? -a : a;
            EXPECT(memcmp(&want, &b, 8) == 0);
        }
    }
    return R;
}

// ---- the reference: the unique edge set, Kruskal in (w, lo, hi) order, depth-first propagation, the vote
static Result run_kruskal(const Case& in) {
    const int64_t n = in.n;
    Result R;
    std::vector<uint8_t> live(n);
    for (int64_t v = 0; v < n; ++v) live[v] = isfinite(in.nrm[v * 3]) && isfinite(in.nrm[v * 3 + 1]) && isfinite(in.nrm[v * 3 + 2]);
    std::vector<std::tuple<uint64_t, int64_t, int64_t>> edges;
    for (int64_t v = 0; v < n; ++v) {
        if (!live[v]) continue;
        const int32_t len = std::min(std::max(in.count[v], 0), in.stride);
        for (int32_t k = 0; k < len; ++k) {
            const int64_t j = in.nbr[v * in.stride + k];
            if (j < 0 || j >= n || j == v || !live[j]) continue;
            const int64_t lo = std::min(v, j), hi = std::max(v, j);
            const double dot = in.nrm[lo * 3] * in.nrm[hi * 3] + in.nrm[lo * 3 + 1] * in.nrm[hi * 3 + 1] + in.nrm[lo * 3 + 2] * in.nrm[hi * 3 + 2];
            edges.emplace_back(orient_key(dot), lo, hi);
        }
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<int64_t> uf(n);
    for (int64_t v = 0; v < n; ++v) uf[v] = v;
    auto find = [&](int64_t v) { while (uf[v] != v) { uf[v] = uf[uf[v]]; v = uf[v]; } return v; };
    std::vector<std::vector<std::pair<int64_t, int>>> tree(n);
    for (auto& [w, lo, hi] : edges) {
        const int64_t a = find(lo), b = find(hi);
        if (a == b) continue;
        uf[a] = b;
        const double dot = in.nrm[lo * 3] * in.nrm[hi * 3] + in.nrm[lo * 3 + 1] * in.nrm[hi * 3 + 1] + in.nrm[lo * 3 + 2] * in.nrm[hi * 3 + 2];
        tree[lo].push_back({hi, dot < 0.0});
        tree[hi].push_back({lo, dot < 0.0});
    }
    R.flip.assign(n, 0);
    R.component.assign(n, -1);
    std::vector<int64_t> stack;
    for (int64_t s = 0; s < n; ++s) {
        if (R.component[s] >= 0) continue;
        ++R.n_components;
        if (!live[s]) { ++R.n_not_live; R.component[s] = (int32_t)s; continue; }
        std::vector<int64_t> members;
        R.component[s] = (int32_t)s;
        stack.push_back(s);
        while (!stack.empty()) {
            const int64_t v = stack.back();
            stack.pop_back();
            members.push_back(v);
            for (auto [j, neg] : tree[v])
                if (R.component[j] < 0) { R.component[j] = (int32_t)s; R.flip[j] = R.flip[v] ^ (uint8_t)neg; stack.push_back(j); }
        }
        if (in.vote) {
            int64_t toward = 0, away = 0;
            for (int64_t v : members) {
                const double px = in.xyz[v * 3], py = in.xyz[v * 3 + 1], pz = in.xyz[v * 3 + 2];
                if (!(isfinite(px) && isfinite(py) && isfinite(pz))) continue;
                const double s2 = R.flip[v] ? -1.0 : 1.0;
                const double t = (in.c[0] - px) * (s2 * in.nrm[v * 3]) + (in.c[1] - py) * (s2 * in.nrm[v * 3 + 1]) + (in.c[2] - pz) * (s2 * in.nrm[v * 3 + 2]);
                toward += t > 0.0; away += t < 0.0;
            }
            if (away > toward) for (int64_t v : members) R.flip[v] ^= 1;
        }
        for (int64_t v : members) R.n_flipped += R.flip[v];
    }
    return R;
}

static void compare(const char* name, const Case& c, int want_rounds = -1) {
    const Result a = run_steps(c), b = run_kruskal(c);
    EXPECT(a.ok);
    if (!a.ok) { printf("  case %s: the rounds did not end in a flat forest\n", name); return; }
    EXPECT(a.flip == b.flip);
    EXPECT(a.component == b.component);
    EXPECT(a.n_components == b.n_components && a.n_flipped == b.n_flipped && a.n_not_live == b.n_not_live);
    EXPECT(a.rounds <= 31);
    if (want_rounds >= 0) EXPECT(a.rounds == want_rounds);
    printf("  %-12s n %6lld  components %5lld  flipped %6lld  dead %3lld  rounds %d\n", name, (long long)c.n, (long long)a.n_components,
           (long long)a.n_flipped, (long long)a.n_not_live, a.rounds);
}

static Case random_case(std::mt19937_64& rng, int64_t n, int32_t stride, int quantum, bool junk, bool vote) {
    Case c;
    c.n = n; c.stride = stride; c.vote = vote;
    c.c[0] = 0.1; c.c[1] = -0.2; c.c[2] = 0.3;
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    c.xyz.resize(n * 3); c.nrm.resize(n * 3); c.nbr.assign(n * stride, -7); c.count.resize(n);
    for (int64_t v = 0; v < n; ++v) {
        for (int k = 0; k < 3; ++k) c.xyz[v * 3 + k] = (float)U(rng);
        // quantum > 0: components on a coarse lattice, so many weights tie exactly
        for (int k = 0; k < 3; ++k) c.nrm[v * 3 + k] = quantum ? (double)((int)(rng() % (2 * quantum + 1)) - quantum) / quantum : U(rng);
        if (junk && rng() % 23 == 0) c.nrm[v * 3 + (int)(rng() % 3)] = rng() % 2 ? NAN : INFINITY;
        if (junk && rng() % 31 == 0) c.xyz[v * 3] = NAN;
        int32_t len = (int32_t)(rng() % (stride + 1));
        if (junk && rng() % 11 == 0) len = (int32_t)(rng() % 3) - 1 + (rng() % 2 ? stride + 2 : 0);      // -1 .. 1, or past the row
        c.count[v] = len;
        for (int32_t k = 0; k < stride; ++k) {
            int64_t j = (int64_t)(rng() % (uint64_t)n);
            if (n > 64 && rng() % 2) j = (v + (int64_t)(rng() % 9) - 4 + n) % n;                           // local: long thin components
            if (junk) switch (rng() % 12) {
                case 0: j = v; break;
                case 1: j = -1; break;
                case 2: j = n; break;
                case 3: j = 2147483647; break;
                case 4: j = k ? c.nbr[v * stride + k - 1] : v; break;                                     // a duplicate
                default: break;
            }
            c.nbr[v * stride + k] = (int32_t)j;
        }
    }
    return c;
}

// a line whose weights strictly increase: one round hooks vertex i to i - 1, a chain of depth n - 1; half the signs flipped
static Case chain_case(std::mt19937_64& rng, int64_t n) {
    Case c;
    c.n = n; c.stride = 3; c.vote = false;
    c.c[0] = c.c[1] = c.c[2] = 0.0;
    c.xyz.assign(n * 3, 0.0f); c.nrm.resize(n * 3); c.nbr.resize(n * 3); c.count.assign(n, 3);
    double angle = 0.0;
    for (int64_t v = 0; v < n; ++v) {
        angle += 1e-3 + (double)v / (double)n;                         // increments that grow with v, below a right angle
        const double s = rng() % 2 ? -1.0 : 1.0;
        c.xyz[v * 3] = (float)v;
        c.nrm[v * 3] = s * cos(angle); c.nrm[v * 3 + 1] = s * sin(angle); c.nrm[v * 3 + 2] = 0.0;
        c.nbr[v * 3] = (int32_t)v; c.nbr[v * 3 + 1] = (int32_t)(v - 1); c.nbr[v * 3 + 2] = (int32_t)(v + 1 < n ? v + 1 : -1);
    }
    return c;
}

int main() {
    std::mt19937_64 rng(20240607);
    EXPECT(orient_key(0.0) > orient_key(0.5) && orient_key(0.5) > orient_key(1.0) && orient_key(1.0) > orient_key(1.5));      // w = 1, 0.5, 0, -0.5
    EXPECT(orient_key(-0.5) == orient_key(0.5) && orient_key(NAN) == ORIENT_KEY_NAN && orient_key(INFINITY) < ORIENT_KEY_NAN);
    EXPECT(orient_jump_launches(1) == 2 && orient_jump_launches(32) == 2 && orient_jump_launches(33) == 3 && orient_jump_launches(4096) == 4);
    for (int64_t n : {1, 2, 3, 5, 17}) {
        for (int rep = 0; rep < 20; ++rep) compare("tiny", random_case(rng, n, 1 + (int32_t)(rng() % 4), rep % 2 ? 2 : 0, rep % 3 == 0, rep % 2 == 0));
    }
    compare("random", random_case(rng, 1000, 6, 0, false, true));
    compare("ties", random_case(rng, 1500, 5, 2, false, true));
    compare("all-tied", random_case(rng, 800, 4, 1, false, false));
    compare("junk", random_case(rng, 2000, 7, 3, true, true));
    compare("junk-sparse", random_case(rng, 3000, 2, 0, true, false));
    compare("chain", chain_case(rng, 4096), 1);
    compare("chain-odd", chain_case(rng, 33 * 33 + 5), 1);
    compare("chain-long", chain_case(rng, 40000), 1);
    {
        // the argument check
        const double ref_bad[3] = {0.0, NAN, 0.0}, ref[3] = {0.0, 0.0, 0.0}, nrm[3] = {0, 0, 1};
        const float xyz[3] = {0, 0, 0};
        const int32_t nbr[1] = {0}, cnt[1] = {1};
        EXPECT(orient_check_args(xyz, nrm, 1, nbr, 1, cnt, ref) == nullptr);
        EXPECT(orient_check_args(nullptr, nrm, 1, nbr, 1, cnt, nullptr) == nullptr);
        EXPECT(orient_check_args(nullptr, nullptr, 0, nullptr, 1, nullptr, nullptr) == nullptr);
        EXPECT(orient_check_args(nullptr, nrm, 1, nbr, 1, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, 1, nbr, 1, cnt, ref_bad) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, -1, nbr, 1, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, (int64_t)1 << 31, nbr, 1, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, 1, nbr, 0, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, (int64_t)1 << 29, nbr, 2, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nullptr, 1, nbr, 1, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, 1, nullptr, 1, cnt, ref) != nullptr);
        EXPECT(orient_check_args(xyz, nrm, 1, nbr, 1, nullptr, ref) != nullptr);
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
