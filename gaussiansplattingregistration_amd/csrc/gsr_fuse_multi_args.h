// gsr_fuse_multi_args.h -- the argument checks of gsr_fuse_multi (csrc/fuse_multi.hip): host code only, no HIP, so that a
// stand-alone program can run them under the host sanitizers (scripts/fuse_multi_args_selftest.cpp).
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gsr_hip.h"

namespace gsr {

#define FM_NARR 7

inline float* fm_array(const gsr_model_view* v, int k) {      // (xyz, cov6, dc, sh, opacity, scaling, rot)
    return k == 0 ? v->xyz : k == 1 ? v->cov6 : k == 2 ? v->dc : k == 3 ? v->sh : k == 4 ? v->opacity : k == 5 ? v->scaling : v->rot;
}

inline bool fm_ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// NULL, or the reason the call is refused.  On success: off[m] = the global index of model m's row 0 (off[n_models] = n_total),
// width[k] = floats per row of array k, used[k] = the call carries it, *with_sr = the models carry scaling / rot.
inline const char* fuse_multi_check_args(const gsr_model_view* models, int32_t n_models, int32_t K, const gsr_fuse_params* params, const gsr_model_view* out,
                                         const int32_t* group_of, const gsr_fuse_multi_report* report, int64_t off[GSR_FUSE_MAX_MODELS + 1],
                                         size_t width[FM_NARR], bool used[FM_NARR], bool* with_sr, char* buf, size_t nbuf) {
    if (!models || !params || !out || !report) return "NULL argument";
    if (n_models < 1 || n_models > GSR_FUSE_MAX_MODELS) { snprintf(buf, nbuf, "n_models = %d (must be in [1, %d])", n_models, GSR_FUSE_MAX_MODELS); return buf; }
    if (K != 0 && K != 3 && K != 8 && K != 15) { snprintf(buf, nbuf, "K = %d (must be 0, 3, 8 or 15)", K); return buf; }
    if (!(params->max_distance > 0.0 && params->max_distance <= DBL_MAX)) return "max_distance must be positive and finite";
    if (!(params->kld_max >= 0.0) || !(params->color_delta >= 0.0)) return "kld_max and color_delta must be >= 0";
    const int N = n_models;
    off[0] = 0;
    int sr_state = -1;                                          // of the models that have rows: -1 none seen, 0 without, 1 with scaling / rot
    for (int m = 0; m < N; ++m) {
        const gsr_model_view* v = models + m;
        if (v->n < 0 || v->n >= ((int64_t)1 << 31)) return "row counts must be in [0, 2^31)";
        off[m + 1] = off[m] + v->n;
        if ((v->scaling != nullptr) != (v->rot != nullptr)) return "scaling and rot come together";
        if (v->n > 0 && (!v->xyz || !v->cov6 || !v->dc || !v->opacity || (K > 0 && !v->sh))) return "NULL array in an input model";
        if (v->n > 0) {                                         // an empty model has no arrays to carry: the others decide
            const int sr = v->scaling && v->rot ? 1 : 0;
            if (sr_state >= 0 && sr != sr_state) return "scaling / rot present in some models only";
            sr_state = sr;
        }
    }
    const int64_t n = off[N];
    if (n >= ((int64_t)1 << 31) || n * N >= ((int64_t)1 << 31)) {
        snprintf(buf, nbuf, "%lld rows in %d models: n_total and n_total * n_models must be below 2^31", (long long)n, N);
        return buf;
    }
    *with_sr = sr_state == 1;
    if (out->n < n) { snprintf(buf, nbuf, "the output holds %lld rows, %lld are needed", (long long)out->n, (long long)n); return buf; }
    if (n > 0 && (!out->xyz || !out->cov6 || !out->dc || !out->opacity || (K > 0 && !out->sh) || (*with_sr && (!out->scaling || !out->rot))))
        return "NULL array in the output model";
    const size_t w[FM_NARR] = {3, 6, 3, 3 * (size_t)K, 1, 3, 4};
    for (int k = 0; k < FM_NARR; ++k) { width[k] = w[k]; used[k] = k == 3 ? K > 0 : k >= 5 ? *with_sr : true; }
    const char* overlap = "an output array overlaps another array of the call (the fusion is not in place)";
    for (int i = 0; i < FM_NARR; ++i) {
        if (!used[i]) continue;
        const size_t bo = (size_t)n * w[i] * 4;
        const float* po = fm_array(out, i);
        if (fm_ranges_overlap(po, bo, group_of, (size_t)n * 4)) return overlap;
        for (int j = 0; j < FM_NARR; ++j) {
            if (!used[j]) continue;
            if (i < j && fm_ranges_overlap(po, bo, fm_array(out, j), (size_t)n * w[j] * 4)) return overlap;
            for (int m = 0; m < N; ++m)
                if (fm_ranges_overlap(po, bo, fm_array(models + m, j), (size_t)models[m].n * w[j] * 4)) return overlap;
        }
    }
    if (group_of)
        for (int j = 0; j < FM_NARR; ++j)
            for (int m = 0; used[j] && m < N; ++m)
                if (fm_ranges_overlap(group_of, (size_t)n * 4, fm_array(models + m, j), (size_t)models[m].n * w[j] * 4)) return "group_of overlaps an input array";
    return nullptr;
}

}  // namespace gsr
