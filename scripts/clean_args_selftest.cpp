// clean_args_selftest.cpp -- the host-only argument checks of gsr_outlier_mask / gsr_model_select (csrc/gsr_clean_args.h) as a
// stand-alone program for the host sanitizers.  No HIP, no device:
//
//     clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/clean_args_selftest.cpp -o clean_args_selftest
//     ./clean_args_selftest
//
// (with hipcc: -x c++ -Xarch_host -fsanitize=address,undefined).  Exit status 0 and "ok" when every check answers as documented.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../gaussiansplattingregistration_amd/csrc/gsr_clean_args.h"

using namespace gsr;

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static gsr_clean_params defaults() {
    gsr_clean_params p;
    memset(&p, 0, sizeof(p));
    p.min_raw_opacity = -INFINITY; p.max_log_scale = INFINITY; p.nb_neighbors = 20; p.std_ratio = 2.0; p.radius = 0.0; p.nb_points = 16;
    return p;
}

int main() {
    const int64_t n = 16;
    std::vector<float> xyz(n * 3, 0.5f), op(n, 0.0f), sc(n * 3, 0.0f);
    std::vector<uint8_t> mask(n, 1);
    gsr_clean_report rep;
    char buf[128];
    auto check = [&](const gsr_clean_params& p, const float* o, const float* s, int64_t rows) {
        return clean_check_args(xyz.data(), o, s, rows, &p, mask.data(), &rep, buf, sizeof(buf));
    };
    gsr_clean_params p = defaults();
    EXPECT(check(p, nullptr, nullptr, n) == nullptr);
    EXPECT(check(p, nullptr, nullptr, 0) == nullptr);
    EXPECT(check(p, nullptr, nullptr, -1) != nullptr);
    EXPECT(check(p, nullptr, nullptr, (int64_t)1 << 31) != nullptr);
    p.nb_neighbors = 33; EXPECT(check(p, nullptr, nullptr, n) && strstr(check(p, nullptr, nullptr, n), "nb_neighbors"));
    p.nb_neighbors = -1; EXPECT(check(p, nullptr, nullptr, n) != nullptr);
    p = defaults(); p.std_ratio = 0.0; EXPECT(check(p, nullptr, nullptr, n) != nullptr);
    p.std_ratio = NAN; EXPECT(check(p, nullptr, nullptr, n) != nullptr);
    p.nb_neighbors = 0; p.std_ratio = 0.0; EXPECT(check(p, nullptr, nullptr, n) == nullptr);
    p = defaults(); p.min_raw_opacity = -2.0; EXPECT(check(p, nullptr, nullptr, n) != nullptr); EXPECT(check(p, op.data(), nullptr, n) == nullptr);
    p = defaults(); p.max_log_scale = 1.0; EXPECT(check(p, nullptr, nullptr, n) != nullptr); EXPECT(check(p, nullptr, sc.data(), n) == nullptr);
    p = defaults(); p.min_raw_opacity = NAN; EXPECT(check(p, op.data(), nullptr, n) != nullptr);
    EXPECT(clean_check_args(nullptr, nullptr, nullptr, n, &p, mask.data(), &rep, buf, sizeof(buf)) != nullptr);
    EXPECT(clean_check_args(xyz.data(), nullptr, nullptr, n, nullptr, mask.data(), &rep, buf, sizeof(buf)) != nullptr);

    // the views: one slab per array, laid out one after the other
    const int K = 3;
    const size_t w[GSR_MODEL_NARR] = {3, 6, 3, 3 * K, 1, 3, 4};
    std::vector<float> in_buf, out_buf;
    size_t off[GSR_MODEL_NARR + 1] = {0};
    for (int k = 0; k < GSR_MODEL_NARR; ++k) off[k + 1] = off[k] + (size_t)n * w[k];
    in_buf.assign(off[GSR_MODEL_NARR], 1.0f);
    out_buf.assign(off[GSR_MODEL_NARR], 0.0f);
    auto view = [&](std::vector<float>& b) {
        gsr_model_view v;
        v.n = n; v.xyz = b.data() + off[0]; v.cov6 = b.data() + off[1]; v.dc = b.data() + off[2]; v.sh = b.data() + off[3];
        v.opacity = b.data() + off[4]; v.scaling = b.data() + off[5]; v.rot = b.data() + off[6];
        return v;
    };
    std::vector<int32_t> index(n);
    int64_t n_out = 0;
    size_t width[GSR_MODEL_NARR];
    bool used[GSR_MODEL_NARR];
    gsr_model_view vi = view(in_buf), vo = view(out_buf);
    EXPECT(select_check_args(&vi, K, mask.data(), &vo, index.data(), &n_out, width, used) == nullptr);
    for (int k = 0; k < GSR_MODEL_NARR; ++k) EXPECT(used[k] && width[k] == w[k]);
    EXPECT(select_check_args(&vi, 0, mask.data(), &vo, nullptr, &n_out, width, used) == nullptr && !used[3]);
    for (int badK : {1, 2, 4, 16, -3}) EXPECT(select_check_args(&vi, badK, mask.data(), &vo, nullptr, &n_out, width, used) != nullptr);
    EXPECT(select_check_args(&vi, K, mask.data(), &vi, nullptr, &n_out, width, used) != nullptr);            // in place
    vo = view(out_buf); vo.cov6 = vi.xyz + 3 * (n - 1);
    EXPECT(select_check_args(&vi, K, mask.data(), &vo, nullptr, &n_out, width, used) != nullptr);            // one row of overlap
    vo = view(out_buf); vo.dc = vo.xyz;
    EXPECT(select_check_args(&vi, K, mask.data(), &vo, nullptr, &n_out, width, used) != nullptr);            // two outputs on one buffer
    vo = view(out_buf);
    EXPECT(select_check_args(&vi, K, mask.data(), &vo, reinterpret_cast<int32_t*>(vo.rot), &n_out, width, used) != nullptr);
    EXPECT(select_check_args(&vi, K, reinterpret_cast<uint8_t*>(vo.opacity), &vo, nullptr, &n_out, width, used) != nullptr);
    vi.rot = nullptr;
    EXPECT(select_check_args(&vi, K, mask.data(), &vo, nullptr, &n_out, width, used) != nullptr);            // scaling without rot
    vi = view(in_buf); vi.n = (int64_t)1 << 31;
    EXPECT(select_check_args(&vi, K, mask.data(), &vo, nullptr, &n_out, width, used) != nullptr);
    vi = view(in_buf); vi.n = 0; vo.n = 0;
    EXPECT(select_check_args(&vi, K, nullptr, &vo, nullptr, &n_out, width, used) == nullptr);                // an empty model
    EXPECT(select_check_args(nullptr, K, mask.data(), &vo, nullptr, &n_out, width, used) != nullptr);
    // adjacent buffers do not overlap
    EXPECT(!ranges_overlap(in_buf.data(), 16, in_buf.data() + 4, 16) && ranges_overlap(in_buf.data(), 17, in_buf.data() + 4, 16));
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
