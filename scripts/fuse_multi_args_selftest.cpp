// fuse_multi_args_selftest.cpp -- the host-only argument checks of gsr_fuse_multi, gsr_model_fuse and gsr_model_match
// (csrc/gsr_fuse_args.h) as a stand-alone program for the host sanitizers:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/fuse_multi_args_selftest.cpp -o fuse_multi_args_selftest
//     ./fuse_multi_args_selftest
//
// Prints "ok" and returns 0, or says which case went wrong.
#include <math.h>
#include <string.h>

#include <vector>

#include "../gaussiansplattingregistration_amd/csrc/gsr_fuse_args.h"

using namespace gsr;

struct Call {
    static constexpr int N = 3, ROWS = 8, K = 15;
    std::vector<std::vector<float>> store;
    gsr_model_view models[GSR_FUSE_MAX_MODELS + 1];
    gsr_model_view out;
    gsr_fuse_params params{0.25, 0.5, INFINITY};
    gsr_fuse_multi_report report;
    gsr_fuse_report fuse_report;
    std::vector<int32_t> group_of;
    float* arr(size_t n) { store.emplace_back(n, 0.5f); return store.back().data(); }
    void fill(gsr_model_view* v, int64_t rows, bool sr) {
        memset(v, 0, sizeof(*v));
        v->n = rows;
        v->xyz = arr(rows * 3); v->cov6 = arr(rows * 6); v->dc = arr(rows * 3); v->sh = arr(rows * 3 * K); v->opacity = arr(rows);
        if (sr) { v->scaling = arr(rows * 3); v->rot = arr(rows * 4); }
    }
    explicit Call(bool sr = false) : group_of(N * ROWS) {
        store.reserve(256);
        for (int m = 0; m < N; ++m) fill(models + m, ROWS, sr);
        fill(&out, N * ROWS, sr);
    }
    const char* check(int n_models = N, int k = K) {
        int64_t off[GSR_FUSE_MAX_MODELS + 1];
        size_t width[GSR_MODEL_NARR];
        bool used[GSR_MODEL_NARR], with_sr = false;
        char buf[256];
        const char* r = fuse_multi_check_args(models, n_models, k, &params, &out, group_of.data(), &report, off, width, used, &with_sr, buf, sizeof buf);
        if (!r && off[n_models] != (int64_t)n_models * ROWS) return "wrong offsets";
        return r ? "refused" : nullptr;
    }
    bool fuse_raw(const gsr_model_view* a, const gsr_model_view* b, const gsr_fuse_params* p, const gsr_model_view* o, const gsr_fuse_report* r, int k = K,
                  const int32_t* pairs = nullptr) {      // true: refused
        size_t width[GSR_MODEL_NARR];
        bool used[GSR_MODEL_NARR], with_sr = false;
        char buf[256];
        return fuse_check_args(a, b, k, p, o, pairs, r, width, used, &with_sr, buf, sizeof buf) != nullptr;
    }
    bool fuse(int k = K, const int32_t* pairs = nullptr) { return fuse_raw(models, models + 1, &params, &out, &fuse_report, k, pairs); }
    bool match() { return match_check_args(models, models + 1, &params, &fuse_report) != nullptr; }
};

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("FAILED: %s\n", what); ++failures; } } while (0)

int main() {
    { Call c; EXPECT(!c.check(), "a valid call"); }
    { Call c(true); EXPECT(!c.check(), "a valid call with scaling / rot"); }
    { Call c; EXPECT(!c.check(1) && !c.check(2), "fewer models"); }
    for (int n : {-1, 0, 17, 1 << 30}) { Call c; EXPECT(c.check(n), "n_models out of range"); }
    for (int k : {-1, 1, 2, 4, 16}) { Call c; EXPECT(c.check(Call::N, k), "K"); }
    for (double r : {0.0, -1.0, (double)INFINITY, (double)NAN}) { Call c; c.params.max_distance = r; EXPECT(c.check(), "max_distance"); }
    { Call c; c.params.kld_max = NAN; EXPECT(c.check(), "kld_max NaN"); }
    { Call c; c.params.color_delta = -1.0; EXPECT(c.check(), "color_delta < 0"); }
    { Call c; c.models[2].cov6 = nullptr; EXPECT(c.check(), "NULL input array"); }
    { Call c; c.out.opacity = nullptr; EXPECT(c.check(), "NULL output array"); }
    { Call c(true); c.models[1].scaling = nullptr; EXPECT(c.check(), "scaling without rot"); }
    { Call c(true); c.models[1].scaling = c.models[1].rot = nullptr; EXPECT(c.check(), "mixed array sets"); }
    { Call c; c.models[0].n = (int64_t)1 << 31; EXPECT(c.check(), "row count 2^31"); }
    { Call c; c.models[2].n = -1; EXPECT(c.check(), "negative row count"); }
    { Call c; c.out.n = 23; EXPECT(c.check(), "capacity below n_total"); }
    { Call c; c.out.xyz = c.models[2].xyz; EXPECT(c.check(), "output on an input"); }
    { Call c; c.out.sh = c.models[1].sh + 4; EXPECT(c.check(), "output inside an input"); }
    { Call c; c.out.dc = c.out.xyz + 3; EXPECT(c.check(), "two outputs overlap"); }
    {   // an empty model among full ones carries no arrays and decides nothing
        Call c(true);
        memset(&c.models[1], 0, sizeof(gsr_model_view));
        int64_t off[GSR_FUSE_MAX_MODELS + 1];
        size_t width[GSR_MODEL_NARR];
        bool used[GSR_MODEL_NARR], with_sr = false;
        char buf[256];
        const char* r = fuse_multi_check_args(c.models, 3, 15, &c.params, &c.out, nullptr, &c.report, off, width, used, &with_sr, buf, sizeof buf);
        EXPECT(!r && with_sr && off[1] == 8 && off[2] == 8 && off[3] == 16 && used[5] && used[6] && width[3] == 45, "an empty model among full ones");
    }
    {   // n_total * n_models must stay below 2^31: 16 models of 2^27 rows (the arrays are never touched by the checks up to there)
        Call c;
        for (int m = 0; m < 16; ++m) { c.models[m] = c.models[0]; c.models[m].n = (int64_t)1 << 27; }
        c.out.n = (int64_t)1 << 31;
        EXPECT(c.check(16), "n_total * n_models >= 2^31");
    }
    // ---- the pairwise calls: gsr_model_fuse over models[0] and models[1] into `out`, gsr_model_match over the same two
    { Call c(true); EXPECT(!c.fuse() && !c.fuse(0) && !c.fuse(Call::K, c.group_of.data()) && !c.match(), "valid pairwise calls"); }
    {
        Call c;
        const gsr_model_view *a = c.models, *b = c.models + 1;
        EXPECT(c.fuse_raw(nullptr, b, &c.params, &c.out, &c.fuse_report) && c.fuse_raw(a, nullptr, &c.params, &c.out, &c.fuse_report) &&
               c.fuse_raw(a, b, nullptr, &c.out, &c.fuse_report) && c.fuse_raw(a, b, &c.params, nullptr, &c.fuse_report) &&
               c.fuse_raw(a, b, &c.params, &c.out, nullptr), "pairwise NULL a, b, params, out, report");
        EXPECT(match_check_args(nullptr, b, &c.params, &c.fuse_report) && match_check_args(a, b, &c.params, nullptr), "match: NULL argument");
    }
    for (int k : {-1, 1, 2, 4, 16}) { Call c; EXPECT(c.fuse(k), "pairwise K"); }
    for (double r : {0.0, -1.0, (double)INFINITY, (double)NAN}) { Call c; c.params.max_distance = r; EXPECT(c.fuse() && c.match(), "pairwise max_distance"); }
    for (double k : {-0.1, (double)NAN}) { Call c; c.params.kld_max = k; EXPECT(c.fuse() && c.match(), "pairwise kld_max"); }
    { Call c; c.params.color_delta = -1.0; EXPECT(c.fuse() && c.match(), "pairwise color_delta < 0"); }
    for (float* gsr_model_view::*f : {&gsr_model_view::xyz, &gsr_model_view::cov6, &gsr_model_view::dc, &gsr_model_view::sh, &gsr_model_view::opacity}) {
        { Call c; c.models[0].*f = nullptr; EXPECT(c.fuse() && (c.match() || f == &gsr_model_view::sh), "pairwise NULL input array (match reads no sh)"); }
        { Call c; c.out.*f = nullptr; EXPECT(c.fuse(), "pairwise NULL output array"); }
    }
    { Call c(true); c.models[1].scaling = nullptr; EXPECT(c.fuse(), "pairwise scaling without rot"); }
    { Call c(true); c.models[1].scaling = c.models[1].rot = nullptr; EXPECT(c.fuse(), "pairwise scaling / rot on one side only"); }
    { Call c(true); c.out.scaling = c.out.rot = nullptr; EXPECT(c.fuse(), "pairwise output without scaling / rot"); }
    { Call c; c.models[0].n = (int64_t)1 << 31; EXPECT(c.fuse() && c.match(), "pairwise row count 2^31"); }
    { Call c; c.models[1].n = -1; EXPECT(c.fuse() && c.match(), "pairwise negative row count"); }
    { Call c; c.out.n = 15; EXPECT(c.fuse(), "pairwise capacity below na + nb"); }
    { Call c; c.out.xyz = c.models[0].xyz; EXPECT(c.fuse(), "pairwise output on an input"); }
    { Call c; c.out.sh = c.models[1].sh + 4; EXPECT(c.fuse(), "pairwise output inside an input"); }
    { Call c; c.out.dc = c.out.xyz + 3; EXPECT(c.fuse(), "pairwise two outputs overlap"); }
    { Call c; EXPECT(c.fuse(Call::K, reinterpret_cast<int32_t*>(c.out.cov6)), "the pair list on an output"); }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
