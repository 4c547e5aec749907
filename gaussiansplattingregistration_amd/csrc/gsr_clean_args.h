// gsr_clean_args.h -- the argument checks of gsr_outlier_mask and gsr_model_select (csrc/clean.hip): host code only, no HIP, so
// that a stand-alone program can run them under the host sanitizers (scripts/clean_args_selftest.cpp).  Each returns NULL or the
// reason the call is refused.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gsr_hip.h"

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

inline bool clean_ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

#define GSR_SELECT_NARR 7
// width[k] = floats per row of array k (xyz, cov6, dc, sh, opacity, scaling, rot); used[k] = the call carries it
inline const char* select_check_args(const gsr_model_view* in, int32_t K, const uint8_t* mask, const gsr_model_view* out, const int32_t* index,
                                     const int64_t* n_out, size_t width[GSR_SELECT_NARR], bool used[GSR_SELECT_NARR]) {
    if (!in || !out || !n_out) return "NULL argument";
    if (K != 0 && K != 3 && K != 8 && K != 15) return "K must be 0, 3, 8 or 15";
    if (in->n < 0 || in->n >= ((int64_t)1 << 31)) return "row count must lie in [0, 2^31)";
    if (out->n < 0) return "negative output capacity";
    if (in->n > 0 && !mask) return "NULL mask";
    if ((in->scaling != nullptr) != (in->rot != nullptr)) return "scaling and rot come together";
    const size_t w[GSR_SELECT_NARR] = {3, 6, 3, 3 * (size_t)K, 1, 3, 4};
    const float* pi[GSR_SELECT_NARR] = {in->xyz, in->cov6, in->dc, in->sh, in->opacity, in->scaling, in->rot};
    float* po[GSR_SELECT_NARR] = {out->xyz, out->cov6, out->dc, out->sh, out->opacity, out->scaling, out->rot};
    const size_t ni = (size_t)in->n, no = (size_t)out->n;
    for (int k = 0; k < GSR_SELECT_NARR; ++k) {
        width[k] = w[k];
        used[k] = pi[k] != nullptr && w[k] > 0;
        if (used[k] && !po[k] && no > 0 && ni > 0) return "an array of the input has no place in the output";
    }
    for (int i = 0; i < GSR_SELECT_NARR; ++i) {
        if (!used[i]) continue;
        const size_t bo = no * w[i] * 4;
        if (clean_ranges_overlap(po[i], bo, mask, ni) || clean_ranges_overlap(po[i], bo, index, no * 4))
            return "an output array overlaps another array of the call (the selection is not in place)";
        for (int j = 0; j < GSR_SELECT_NARR; ++j) {
            if (!used[j]) continue;
            if (clean_ranges_overlap(po[i], bo, pi[j], ni * w[j] * 4) || (i < j && clean_ranges_overlap(po[i], bo, po[j], no * w[j] * 4)))
                return "an output array overlaps another array of the call (the selection is not in place)";
        }
    }
    if (index) {
        if (clean_ranges_overlap(index, no * 4, mask, ni)) return "index overlaps the mask";
        for (int j = 0; j < GSR_SELECT_NARR; ++j)
            if (used[j] && clean_ranges_overlap(index, no * 4, pi[j], ni * w[j] * 4)) return "index overlaps an input array";
    }
    return nullptr;
}

}  // namespace gsr
