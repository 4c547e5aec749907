// gsr_clean_args.h -- the argument checks of gsr_outlier_mask and gsr_model_select (csrc/clean.hip): host code only, no HIP, so
// that a stand-alone program can run them under the host sanitizers (scripts/clean_args_selftest.cpp).  Each returns NULL or the
// reason the call is refused.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "gsr_model_arrays.h"

namespace gsr {

#define GSR_CLEAN_MAX_NN 32

inline const char* clean_check_args(const float* xyz, const float* raw_opacity, const float* scaling, int64_t n, const gsr_clean_params* p,
                                    const uint8_t* mask, const gsr_clean_report* report, char* buf, size_t nbuf) {
    if (!p || !report) return "NULL params or report";
    if (n < 0 || n >= ((int64_t)1 << 31)) { snprintf(buf, nbuf, "n = %lld (must lie in [0, 2^31))", (long long)n); return buf; }
    if (n > 0 && (!xyz || !mask)) return "NULL xyz or mask";
    if (p->nb_neighbors < 0 || p->nb_neighbors > GSR_CLEAN_MAX_NN) {
        snprintf(buf, nbuf, "nb_neighbors = %d (must lie in [0, %d])", p->nb_neighbors, GSR_CLEAN_MAX_NN);
        return buf;
    }
    if (p->nb_neighbors >= 1 && !(p->std_ratio > 0.0)) return "std_ratio must be > 0 when the statistical stage is on";
    if (p->min_raw_opacity != p->min_raw_opacity || p->max_log_scale != p->max_log_scale) return "a gate threshold is NaN";
    if (p->min_raw_opacity > -1.0 / 0.0 && !raw_opacity) return "the opacity gate is on (min_raw_opacity > -inf) without raw_opacity";
    if (p->max_log_scale < 1.0 / 0.0 && !scaling) return "the scale gate is on (max_log_scale < +inf) without scaling";
    if (p->radius > 0.0 && p->nb_points < 0) return "nb_points must be >= 0";
    return nullptr;
}

// width[k] = floats per row of array k; used[k] = the input has the array (a selection carries whatever arrays its input has)
inline const char* select_check_args(const gsr_model_view* in, int32_t K, const uint8_t* mask, const gsr_model_view* out, const int32_t* index,
                                     const int64_t* n_out, size_t width[GSR_MODEL_NARR], bool used[GSR_MODEL_NARR]) {
    if (!in || !out || !n_out) return "NULL argument";
    if (!sh_count_ok(K)) return "K must be 0, 3, 8 or 15";
    if (const char* why = model_check_input(in, K, false)) return why;
    if (out->n < 0) return "negative output capacity";
    if (in->n > 0 && !mask) return "NULL mask";
    const size_t ni = (size_t)in->n, no = (size_t)out->n;
    model_layout(K, true, width, used);
    for (int k = 0; k < GSR_MODEL_NARR; ++k) {
        used[k] = used[k] && model_array(in, k) != nullptr;
        if (used[k] && !model_array(out, k) && no > 0 && ni > 0) return "an array of the input has no place in the output";
    }
    const ByteRange extra[2] = {{mask, ni}, {index, no * 4}};
    if (!model_outputs_disjoint(out, no, used, width, &in, 1, extra, 2))
        return "an output array overlaps another array of the call (the selection is not in place)";
    ByteRange read[GSR_MODEL_NARR + 1];
    int n_read = model_ranges(in, ni, used, width, read, 0);
    read[n_read++] = extra[0];
    if (!outputs_disjoint(&extra[1], 1, read, n_read)) return "index overlaps the mask or an input array";
    return nullptr;
}

}  // namespace gsr
