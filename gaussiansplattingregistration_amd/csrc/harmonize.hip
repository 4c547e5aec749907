// harmonize.hip -- colour harmonisation of registered scenes (gsr_color_sums, gsr_color_solve, gsr_model_color_apply;
// include/gsr_hip.h).  The definitions are restated in float64 in tests/color_model.py.
//
//   k_color_sums      a lane per pair, grid-stride: the two gathers (dc, opacity of either side), the residual at the current
//                     transforms, the Huber weight, 39 float64 sums in registers, folded by block_fold_store and k_fold_partials
//                     (gsr_fold.h, the xor tree).  The two counts are integer atomics.
//   k_color_apply     a lane per colour triple of the model (n DC triples, then n K SH triples): float64, narrowed once.
// gsr_color_solve is host code (csrc/gsr_colorsolve.h); gsr_model_match, the pair list, lives beside gsr_model_fuse in fuse.hip.
#include "gsr_common.h"
#include "gsr_fold.h"
#include "gsr_oneshot.h"
#include "gsr_colorsolve.h"

#include <float.h>
#include <math.h>
#include <string.h>

namespace gsr {

#define COLOR_C0 0.28209479177387814
#define COLOR_NACC 39
struct ColorXf { double m[12]; };

__device__ __forceinline__ bool color_finite(float v) { return fabsf(v) <= FLT_MAX; }

__global__ __launch_bounds__(256) void k_color_sums(int64_t n_pairs, const int32_t* __restrict__ pairs, const float* __restrict__ s_dc,
                                                    const float* __restrict__ s_op, int64_t ns, const float* __restrict__ t_dc,
                                                    const float* __restrict__ t_op, int64_t nt, ColorXf Ps, ColorXf Pt, double huber_k,
                                                    double* __restrict__ partials, unsigned long long* __restrict__ counters) {
    double acc[COLOR_NACC];
#pragma unroll
    for (int k = 0; k < COLOR_NACC; ++k) acc[k] = 0.0;
    unsigned skipped = 0, outside = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = pairs[2 * p], j = pairs[2 * p + 1];
        const bool inside = i >= 0 && i < ns && j >= 0 && j < nt;
        float f0 = 0.f, f1 = 0.f, f2 = 0.f, fo = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, go = 0.f;
        if (inside) {                                           // a row outside its model is never dereferenced
            f0 = s_dc[3 * i]; f1 = s_dc[3 * i + 1]; f2 = s_dc[3 * i + 2]; fo = s_op[i];
            g0 = t_dc[3 * j]; g1 = t_dc[3 * j + 1]; g2 = t_dc[3 * j + 2]; go = t_op[j];
        }
        const bool finite = color_finite(f0) && color_finite(f1) && color_finite(f2) && color_finite(fo) && color_finite(g0) && color_finite(g1) &&
                            color_finite(g2) && color_finite(go);
        outside += inside ? 0u : 1u;
        skipped += inside && !finite ? 1u : 0u;
        // no branch around the 39 additions (a divergent `continue` keeps two copies of every accumulator alive): a pair that does not
        // count gets zero inputs and the weight 0, and adds +0.0 everywhere
        const bool ok = inside && finite;
        if (!ok) { f0 = f1 = f2 = fo = g0 = g1 = g2 = go = 0.f; }
        const double a[4] = {0.5 + COLOR_C0 * (double)f0, 0.5 + COLOR_C0 * (double)f1, 0.5 + COLOR_C0 * (double)f2, 1.0};
        const double b[4] = {0.5 + COLOR_C0 * (double)g0, 0.5 + COLOR_C0 * (double)g1, 0.5 + COLOR_C0 * (double)g2, 1.0};
        const double u = (1.0 / (1.0 + exp(-(double)fo))) * (1.0 / (1.0 + exp(-(double)go)));
        double rho2 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double pa = ((Ps.m[4 * c] * a[0] + Ps.m[4 * c + 1] * a[1]) + Ps.m[4 * c + 2] * a[2]) + Ps.m[4 * c + 3];
            const double pb = ((Pt.m[4 * c] * b[0] + Pt.m[4 * c + 1] * b[1]) + Pt.m[4 * c + 2] * b[2]) + Pt.m[4 * c + 3];
            const double r = pa - pb;
            rho2 += r * r;
        }
        const double rho = sqrt(rho2);
        const double w = ok ? (rho > huber_k ? u * (huber_k / rho) : u) : 0.0;
        acc[0] += ok ? 1.0 : 0.0;
        acc[1] += w;
        acc[2] += w * rho2;
        double wa[4], wb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { wa[k] = w * a[k]; wb[k] = w * b[k]; }
        int t = 3;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) acc[t++] += wa[r] * a[c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t++] += wa[r] * b[c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) acc[t++] += wb[r] * b[c];
    }
    for (int o = 32; o > 0; o >>= 1) { skipped += __shfl_xor(skipped, o); outside += __shfl_xor(outside, o); }
    if ((threadIdx.x & 63) == 0) {
        if (skipped) atomicAdd(&counters[0], (unsigned long long)skipped);
        if (outside) atomicAdd(&counters[1], (unsigned long long)outside);
    }
    block_fold_store<COLOR_NACC, GSR_COLOR_SUMS_LEN, wave_sum_xor>(acc, partials, (int)blockIdx.x);
    if (threadIdx.x >= COLOR_NACC && threadIdx.x < GSR_COLOR_SUMS_LEN) partials[(int64_t)blockIdx.x * GSR_COLOR_SUMS_LEN + threadIdx.x] = 0.0;   // the row's padding
}

// X.m[0..8] = M (row-major), X.m[9..11] = the DC offset.  A lane reads its triple before it writes it: in place is safe.
__global__ __launch_bounds__(256) void k_color_apply(int64_t n_dc, int64_t n_total, ColorXf X, const float* dc, const float* sh, float* dc_out,
                                                     float* sh_out) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_total; t += (int64_t)gridDim.x * blockDim.x) {
        const bool is_dc = t < n_dc;
        const float* src = is_dc ? dc + 3 * t : sh + 3 * (t - n_dc);
        float* dst = is_dc ? dc_out + 3 * t : sh_out + 3 * (t - n_dc);
        const double x = (double)src[0], y = (double)src[1], z = (double)src[2];
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = (X.m[3 * c] * x + X.m[3 * c + 1] * y) + X.m[3 * c + 2] * z;
            if (is_dc) v[c] += X.m[9 + c];
        }
        dst[0] = (float)v[0]; dst[1] = (float)v[1]; dst[2] = (float)v[2];
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_color_sums(const float* s_dc, const float* s_opacity, int64_t ns, const float* t_dc, const float* t_opacity, int64_t nt,
                                  const int32_t* pairs, int64_t n_pairs, const double* P_s, const double* P_t, double huber_k, double* sums,
                                  int64_t* n_skipped, int64_t* n_out_of_range, int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_color_sums";
    if (!P_s || !P_t || !sums) return fail(GSR_E_INVALID, "gsr_color_sums: NULL argument");
    if (ns < 0 || nt < 0 || ns >= ((int64_t)1 << 31) || nt >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "gsr_color_sums: row counts must be in [0, 2^31)");
    if (n_pairs < 0 || n_pairs >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "gsr_color_sums: n_pairs must be in [0, 2^31)");
    if (n_pairs > 0 && !pairs) return fail(GSR_E_INVALID, "gsr_color_sums: %lld pairs and no pair array", (long long)n_pairs);
    if ((ns > 0 && (!s_dc || !s_opacity)) || (nt > 0 && (!t_dc || !t_opacity))) return fail(GSR_E_INVALID, "gsr_color_sums: NULL array in a model with rows");
    if (!(huber_k > 0.0)) return fail(GSR_E_INVALID, "gsr_color_sums: huber_k must be positive (inf: least squares)");
    ColorXf Xs, Xt;
    for (int k = 0; k < 12; ++k) {
        if (!(fabs(P_s[k]) <= DBL_MAX) || !(fabs(P_t[k]) <= DBL_MAX)) return fail(GSR_E_INVALID, "gsr_color_sums: a transform is not finite");
        Xs.m[k] = P_s[k]; Xt.m[k] = P_t[k];
    }
    GSR_TRY(open_device(device, who));
    for (int k = 0; k < GSR_COLOR_SUMS_LEN; ++k) sums[k] = 0.0;
    if (n_skipped) *n_skipped = 0;
    if (n_out_of_range) *n_out_of_range = 0;
    if (n_pairs == 0) return GSR_OK;

    unsigned long long hc[2] = {0, 0};
    double hs[GSR_COLOR_SUMS_LEN];
    OneShot os((hipStream_t)stream, on_device != 0, who);
    hipStream_t st = os.st;
    const float *dsdc, *dsop, *dtdc, *dtop;
    const int32_t* dpairs;
    GSR_TRY(os.in(ns > 0 ? s_dc : nullptr, (size_t)ns * 12, &dsdc));
    GSR_TRY(os.in(ns > 0 ? s_opacity : nullptr, (size_t)ns * 4, &dsop));
    GSR_TRY(os.in(nt > 0 ? t_dc : nullptr, (size_t)nt * 12, &dtdc));
    GSR_TRY(os.in(nt > 0 ? t_opacity : nullptr, (size_t)nt * 4, &dtop));
    GSR_TRY(os.in(pairs, (size_t)n_pairs * 8, &dpairs));
    const int nblk = stride_grid(n_pairs);                      // a function of n_pairs alone: the fold's order is too
    double *partials, *dsums;
    unsigned long long* counters;
    GSR_TRY(os.scratch((size_t)nblk * GSR_COLOR_SUMS_LEN * 8, &partials));
    GSR_TRY(os.scratch(GSR_COLOR_SUMS_LEN * 8, &dsums));
    GSR_TRY(os.scratch(2 * 8, &counters));
    GSR_HIP(hipMemsetAsync(counters, 0, 2 * 8, st));
    hipLaunchKernelGGL(k_color_sums, dim3(nblk), dim3(256), 0, st, n_pairs, dpairs, dsdc, dsop, ns, dtdc, dtop, nt, Xs, Xt, huber_k, partials, counters);
    hipLaunchKernelGGL(k_fold_partials<64>, dim3(GSR_COLOR_SUMS_LEN), dim3(64), 0, st, (int64_t)nblk, GSR_COLOR_SUMS_LEN, (const double*)partials, dsums);
    GSR_HIP(hipMemcpyAsync(hs, dsums, sizeof(hs), hipMemcpyDeviceToHost, st));
    GSR_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, st));
    GSR_TRY(os.finish());
    memcpy(sums, hs, sizeof(hs));
    if (n_skipped) *n_skipped = (int64_t)hc[0];
    if (n_out_of_range) *n_out_of_range = (int64_t)hc[1];
    if (hc[1]) return fail(GSR_E_INVALID, "gsr_color_sums: %llu of %lld pairs index a row outside its model (%lld and %lld rows)", hc[1], (long long)n_pairs,
                           (long long)ns, (long long)nt);
    return GSR_OK;
}

extern "C" int32_t gsr_color_solve(int32_t n_nodes, double* P, int32_t n_edges, const gsr_color_edge* edges, int32_t mode, double prior,
                                   int64_t min_pairs, int32_t reference, int32_t* held, gsr_color_solve_result* result) {
    if (n_nodes < 1 || !P) return fail(GSR_E_INVALID, "gsr_color_solve: no nodes (n_nodes %d)", n_nodes);
    if (n_edges < 0 || (n_edges > 0 && !edges)) return fail(GSR_E_INVALID, "gsr_color_solve: %d edges and no edge array", n_edges);
    std::vector<colorsolve::Edge> E((size_t)n_edges);
    for (int k = 0; k < n_edges; ++k) {
        E[k].s = edges[k].source;
        E[k].t = edges[k].target;
        memcpy(E[k].sums, edges[k].sums, sizeof E[k].sums);
    }
    colorsolve::Result r;
    const std::string err = colorsolve::solve(n_nodes, P, E, mode, prior, min_pairs, reference, held, &r);
    if (!err.empty()) return fail(GSR_E_INVALID, "gsr_color_solve: %s", err.c_str());
    if (result) {
        result->E_initial = r.E_initial;
        result->E_final = r.E_final;
        result->pivot_min = r.pivot_min;
        result->pivot_max = r.pivot_max;
        result->n_free = r.n_free;
        result->n_unknowns = r.n_unknowns;
    }
    return GSR_OK;
}

extern "C" int32_t gsr_model_color_apply(const double* P12, int64_t n, int32_t K, const float* dc, const float* sh, float* dc_out, float* sh_out,
                                         int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_model_color_apply";
    if (!P12) return fail(GSR_E_INVALID, "gsr_model_color_apply: NULL transform");
    if (K != 0 && K != 3 && K != 8 && K != 15) return fail(GSR_E_INVALID, "gsr_model_color_apply: K = %d (must be 0, 3, 8 or 15)", K);
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "gsr_model_color_apply: n must be in [0, 2^31)");
    for (int k = 0; k < 12; ++k)
        if (!(fabs(P12[k]) <= DBL_MAX)) return fail(GSR_E_INVALID, "gsr_model_color_apply: the transform is not finite");
    if (n > 0 && (!dc || !dc_out || (K > 0 && (!sh || !sh_out)))) return fail(GSR_E_INVALID, "gsr_model_color_apply: NULL array");
    const size_t bd = (size_t)n * 12, bs = (size_t)n * (size_t)K * 12;
    if ((dc_out != dc && ranges_overlap(dc_out, bd, dc, bd)) || (K > 0 && sh_out != sh && ranges_overlap(sh_out, bs, sh, bs)) ||
        (K > 0 && (ranges_overlap(dc_out, bd, sh, bs) || ranges_overlap(sh_out, bs, dc, bd) || ranges_overlap(dc_out, bd, sh_out, bs))))
        return fail(GSR_E_INVALID, "gsr_model_color_apply: an output partially overlaps another array of the call (exactly in place, or disjoint)");
    ColorXf X;
    for (int c = 0; c < 3; ++c) {
        for (int j = 0; j < 3; ++j) X.m[3 * c + j] = P12[4 * c + j];
        X.m[9 + c] = ((((P12[4 * c] * 0.5 + P12[4 * c + 1] * 0.5) + P12[4 * c + 2] * 0.5) + P12[4 * c + 3]) - 0.5) / COLOR_C0;
    }
    GSR_TRY(open_device(device, who));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, who);
    const float *ddc, *dsh = nullptr;
    float *odc, *osh = nullptr;
    GSR_TRY(os.in(dc, bd, &ddc));
    GSR_TRY(os.out(dc_out, bd, &odc));
    if (K > 0) { GSR_TRY(os.in(sh, bs, &dsh)); GSR_TRY(os.out(sh_out, bs, &osh)); }
    const int64_t total = n * (int64_t)(K + 1);
    hipLaunchKernelGGL(k_color_apply, dim3(stride_grid(total)), dim3(256), 0, os.st, n, total, X, ddc, dsh, odc, osh);
    return os.finish();
}
