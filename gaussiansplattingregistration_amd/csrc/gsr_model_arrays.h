// gsr_model_arrays.h -- the layout of a splat model behind gsr_model_view, once: which arrays there are, how wide their rows are,
// which of them a call carries, what an input model must satisfy, and the rule that no output overlaps anything else in the call.
// Host code only, no HIP, so that the stand-alone selftests (scripts/*_args_selftest.cpp) run it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsr_hip.h"

namespace gsr {

#define GSR_MODEL_NARR 7

inline float* model_array(const gsr_model_view* v, int k) {      // (xyz, cov6, dc, sh, opacity, scaling, rot)
    return k == 0 ? v->xyz : k == 1 ? v->cov6 : k == 2 ? v->dc : k == 3 ? v->sh : k == 4 ? v->opacity : k == 5 ? v->scaling : v->rot;
}

// width[k] = floats per row of array k; used[k] = a call with K SH coefficients, with or without scaling / rot, carries it
inline void model_layout(int32_t K, bool with_sr, size_t width[GSR_MODEL_NARR], bool used[GSR_MODEL_NARR]) {
    const size_t w[GSR_MODEL_NARR] = {3, 6, 3, 3 * (size_t)K, 1, 3, 4};
    for (int k = 0; k < GSR_MODEL_NARR; ++k) { width[k] = w[k]; used[k] = k == 3 ? K > 0 : k >= 5 ? with_sr : true; }
}

inline bool sh_count_ok(int32_t K) { return K == 0 || K == 3 || K == 8 || K == 15; }

// two byte ranges share a byte (an absent or empty range shares none; adjacent ranges do not overlap)
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// NULL, or the reason an input model is refused: its row count, scaling without rot, and -- where the call needs every array of
// its K (`arrays`; a selection takes what there is) -- an array that is missing from a model with rows
inline const char* model_check_input(const gsr_model_view* v, int32_t K, bool arrays = true) {
    if (v->n < 0 || v->n >= ((int64_t)1 << 31)) return "row counts must be in [0, 2^31)";
    if ((v->scaling != nullptr) != (v->rot != nullptr)) return "scaling and rot come together";
    if (arrays && v->n > 0 && (!v->xyz || !v->cov6 || !v->dc || !v->opacity || (K > 0 && !v->sh))) return "NULL array in an input model";
    return nullptr;
}

struct ByteRange { const void* p; size_t bytes; };

// no outs[i] shares a byte with another outs[j] or with any of others[]
inline bool outputs_disjoint(const ByteRange* outs, int n_outs, const ByteRange* others, int n_others) {
    for (int i = 0; i < n_outs; ++i) {
        for (int j = i + 1; j < n_outs; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return false;
        for (int j = 0; j < n_others; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, others[j].p, others[j].bytes)) return false;
    }
    return true;
}

// the used arrays of `v`, `rows` rows of each, appended to r[n ...]; returns the new count
inline int model_ranges(const gsr_model_view* v, size_t rows, const bool used[GSR_MODEL_NARR], const size_t width[GSR_MODEL_NARR], ByteRange* r, int n) {
    for (int k = 0; k < GSR_MODEL_NARR; ++k)
        if (used[k]) r[n++] = {model_array(v, k), rows * width[k] * 4};
    return n;
}

// the used arrays of `out` (`rows` rows each) overlap neither one another, nor a used array of an input model, nor an extra range
// (pairs, group_of, index, mask) of the call
inline bool model_outputs_disjoint(const gsr_model_view* out, size_t rows, const bool used[GSR_MODEL_NARR], const size_t width[GSR_MODEL_NARR],
                                   const gsr_model_view* const* inputs, int n_inputs, const ByteRange* extra, int n_extra) {
    ByteRange outs[GSR_MODEL_NARR], others[GSR_MODEL_NARR * GSR_FUSE_MAX_MODELS + 2];      // (the most input models one call takes)
    if (n_inputs > GSR_FUSE_MAX_MODELS || n_extra > 2) return false;
    const int n_outs = model_ranges(out, rows, used, width, outs, 0);
    int n = 0;
    for (int m = 0; m < n_inputs; ++m) n = model_ranges(inputs[m], (size_t)inputs[m]->n, used, width, others, n);
    for (int e = 0; e < n_extra; ++e) others[n++] = extra[e];
    return outputs_disjoint(outs, n_outs, others, n);
}

}  // namespace gsr
