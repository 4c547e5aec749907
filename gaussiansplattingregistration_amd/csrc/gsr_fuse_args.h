// gsr_fuse_args.h -- the argument checks of gsr_model_fuse, gsr_model_match (csrc/fuse.hip) and gsr_fuse_multi (csrc/fuse_multi.hip):
// host code only, no HIP, so that a stand-alone program can run them under the host sanitizers (scripts/fuse_multi_args_selftest.cpp).
// Each returns NULL or the reason the call is refused.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "gsr_model_arrays.h"

namespace gsr {

// K and the gates, in the order the entry points have always refused them
inline const char* fuse_check_params(int32_t K, const gsr_fuse_params* params, char* buf, size_t nbuf) {
    if (!sh_count_ok(K)) { snprintf(buf, nbuf, "K = %d (must be 0, 3, 8 or 15)", K); return buf; }
    if (!(params->max_distance > 0.0 && params->max_distance <= DBL_MAX)) return "max_distance must be positive and finite";
    if (!(params->kld_max >= 0.0) || !(params->color_delta >= 0.0)) return "kld_max and color_delta must be >= 0";
    return nullptr;
}

// What both merges ask of their input models: each one valid, and one set of arrays among those that have rows.
// On success: off[m] = the global index of model m's row 0 (off[N] = n_total), *with_sr = the models carry scaling / rot.
inline const char* fuse_check_inputs(const gsr_model_view* const* in, int N, int32_t K, int64_t* off, bool* with_sr) {
    int sr_state = -1;                                          // of the models that have rows: -1 none seen, 0 without, 1 with scaling / rot
    off[0] = 0;
    for (int m = 0; m < N; ++m) {
        if (const char* why = model_check_input(in[m], K)) return why;
        off[m + 1] = off[m] + in[m]->n;
        if (in[m]->n > 0) {                                     // an empty model has no arrays to carry: the others decide
            const int sr = in[m]->scaling && in[m]->rot ? 1 : 0;
            if (sr_state >= 0 && sr != sr_state) return "scaling / rot present in some models only";
            sr_state = sr;
        }
    }
    *with_sr = sr_state == 1;
    return nullptr;
}

// ... and of their output: it holds the n rows of all inputs and overlaps nothing, `extra` (pairs or group_of) included.
// On success: width[k] = floats per row of array k, used[k] = the call carries it.
inline const char* fuse_check_output(const gsr_model_view* const* in, int N, int32_t K, bool with_sr, const gsr_model_view* out, int64_t n, ByteRange extra,
                                     size_t width[GSR_MODEL_NARR], bool used[GSR_MODEL_NARR], char* buf, size_t nbuf) {
    if (out->n < n) { snprintf(buf, nbuf, "the output holds %lld rows, %lld are needed", (long long)out->n, (long long)n); return buf; }
    if (n > 0 && (!out->xyz || !out->cov6 || !out->dc || !out->opacity || (K > 0 && !out->sh) || (with_sr && (!out->scaling || !out->rot))))
        return "NULL array in the output model";
    model_layout(K, with_sr, width, used);
    if (!model_outputs_disjoint(out, (size_t)n, used, width, in, N, &extra, 1))
        return "an output array overlaps another array of the call (the fusion is not in place)";
    return nullptr;
}

inline const char* fuse_check_args(const gsr_model_view* a, const gsr_model_view* b, int32_t K, const gsr_fuse_params* params, const gsr_model_view* out,
                                   const int32_t* pairs, const gsr_fuse_report* report, size_t width[GSR_MODEL_NARR], bool used[GSR_MODEL_NARR], bool* with_sr,
                                   char* buf, size_t nbuf) {
    if (!a || !b || !params || !out || !report) return "NULL argument";
    if (const char* why = fuse_check_params(K, params, buf, nbuf)) return why;
    const gsr_model_view* in[2] = {a, b};
    int64_t off[3];
    if (const char* why = fuse_check_inputs(in, 2, K, off, with_sr)) return why;
    const ByteRange pair_list = {pairs, (size_t)(a->n < b->n ? a->n : b->n) * 8};
    return fuse_check_output(in, 2, K, *with_sr, out, off[2], pair_list, width, used, buf, nbuf);
}

inline const char* match_check_args(const gsr_model_view* a, const gsr_model_view* b, const gsr_fuse_params* params, const gsr_fuse_report* report) {
    if (!a || !b || !params || !report) return "NULL argument";
    if (const char* why = fuse_check_params(0, params, nullptr, 0)) return why;
    for (const gsr_model_view* v : {a, b}) {
        gsr_model_view read = *v;                               // the pair list reads xyz, cov6, dc and opacity: the rest of a view is not looked at
        read.sh = read.scaling = read.rot = nullptr;
        if (const char* why = model_check_input(&read, 0)) return why;
    }
    return nullptr;
}

inline const char* fuse_multi_check_args(const gsr_model_view* models, int32_t n_models, int32_t K, const gsr_fuse_params* params, const gsr_model_view* out,
                                         const int32_t* group_of, const gsr_fuse_multi_report* report, int64_t off[GSR_FUSE_MAX_MODELS + 1],
                                         size_t width[GSR_MODEL_NARR], bool used[GSR_MODEL_NARR], bool* with_sr, char* buf, size_t nbuf) {
    if (!models || !params || !out || !report) return "NULL argument";
    if (n_models < 1 || n_models > GSR_FUSE_MAX_MODELS) { snprintf(buf, nbuf, "n_models = %d (must be in [1, %d])", n_models, GSR_FUSE_MAX_MODELS); return buf; }
    if (const char* why = fuse_check_params(K, params, buf, nbuf)) return why;
    const int N = n_models;
    const gsr_model_view* in[GSR_FUSE_MAX_MODELS];
    for (int m = 0; m < N; ++m) in[m] = models + m;
    if (const char* why = fuse_check_inputs(in, N, K, off, with_sr)) return why;
    const int64_t n = off[N];
    if (n >= ((int64_t)1 << 31) || n * N >= ((int64_t)1 << 31)) {
        snprintf(buf, nbuf, "%lld rows in %d models: n_total and n_total * n_models must be below 2^31", (long long)n, N);
        return buf;
    }
    const ByteRange group = {group_of, (size_t)n * 4};
    if (const char* why = fuse_check_output(in, N, K, *with_sr, out, n, group, width, used, buf, nbuf)) return why;
    ByteRange arrays[GSR_MODEL_NARR];
    for (int m = 0; m < N; ++m)
        if (!outputs_disjoint(&group, 1, arrays, model_ranges(in[m], (size_t)in[m]->n, used, width, arrays, 0))) return "group_of overlaps an input array";
    return nullptr;
}

}  // namespace gsr
