// d2d.hip -- mixture-to-mixture registration: every source component against every target component within
// max_corr, weighted by w_i v_j exp(-m / 2) with m the Mahalanobis distance under s^2 (R A_i R' + B_j) + phi I.  No arg-min, no
// correspondence.  The definition is the header comment of include/gsr_hip.h, the pair and row math is gsr_d2d.h (shared with the host
// self-test), tests/d2d_model.py restates both in float64 NumPy.
//   gsr_d2d_create / set_target / set_source   a context owning the target's point grid (GridIndex), the target's covariances and
//                            weights gathered into cell order (k_d2d_gather_target), and the source's three arrays gathered into the
//                            order of the TARGET's cells (GridIndex::sort_by_cell + k_d2d_gather_source), as the ICP sorts its source
//   gsr_d2d_accumulate       k_d2d_accumulate: one lane per source row.  R A R' once, then grid_box_walk over
//                            grid_rings_for_radius(max_corr) rings; per accepted pair the closed-form inverse, one exp and eleven
//                            float64 additions (sum w M, sum w M r, sum w, sum w m); the 27 entries of H and g are formed ONCE per row
//                            from those (J depends on the row only).  A row's 32 values are folded lane -> wave -> block, and the
//                            blocks' partials by k_fold_partials, in the fixed order of gsr_fold.h (the xor tree).  No float atomics:
//                            the grid is ceil(n / 256) blocks whatever the device, so the same inputs give the same bits.
//   gsr_d2d_register         the IRLS loop on the host: accumulate, pivoted LDL' (solve6), T <- dT T
#include "gsr_common.h"
#include "gsr_d2d.h"
#include "gsr_fold.h"
#include "gsr_grid.h"
#include "gsr_oneshot.h"
#include "gsr_solve.h"

#include <math.h>
#include <string.h>

namespace gsr {

constexpr int D2D_LEN = d2d::SUMS_LEN;
struct D2DXform { double m[12]; };      // rows 0..2 of the 4 x 4

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }

// rec[2 j], rec[2 j + 1] = (B0 B1 B2 B3), (B4 B5 v 0) of the target row at sorted position j; v = NaN when any of the seven is not
// finite (the row then fails the one test the pair loop makes on it)
__global__ __launch_bounds__(256) void k_d2d_gather_target(int64_t n, const unsigned* __restrict__ order, const float* __restrict__ cov6,
                                                           const float* __restrict__ weight, float4* __restrict__ rec) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = order[j];
        float B[6];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) { B[k] = cov6[6 * i + k]; ok = ok && finite_f(B[k]); }
        float v = weight ? weight[i] : 1.0f;
        if (!ok || !finite_f(v)) v = __int_as_float(0x7fc00000);
        rec[2 * j] = make_float4(B[0], B[1], B[2], B[3]);
        rec[2 * j + 1] = make_float4(B[4], B[5], v, 0.0f);
    }
}

// p4[k] = (x y z w), A6[6 k ..] = the covariance of the source row that comes k-th in the order of the target's cells; w = NaN when
// any of the ten values is not finite
__global__ __launch_bounds__(256) void k_d2d_gather_source(int64_t n, const unsigned* __restrict__ order, const float* __restrict__ xyz,
                                                           const float* __restrict__ cov6, const float* __restrict__ weight, float4* __restrict__ p4,
                                                           float* __restrict__ A6) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = order[k];
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        bool ok = finite_f(x) && finite_f(y) && finite_f(z);
#pragma unroll
        for (int e = 0; e < 6; ++e) { const float a = cov6[6 * i + e]; A6[6 * k + e] = a; ok = ok && finite_f(a); }
        float w = weight ? weight[i] : 1.0f;
        if (!ok || !finite_f(w)) w = __int_as_float(0x7fc00000);
        p4[k] = make_float4(x, y, z, w);
    }
}

__global__ __launch_bounds__(256) void k_d2d_accumulate(int64_t ns, const float4* __restrict__ p4, const float* __restrict__ A6, D2DXform T, double s2,
                                                        double phi, IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq,
                                                        const float4* __restrict__ rec, int rings, double max_corr2, double* __restrict__ partials) {
    double out[D2D_LEN];
#pragma unroll
    for (int k = 0; k < D2D_LEN; ++k) out[k] = 0.0;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns) {
        const float4 sp = p4[i];
        const double w = (double)sp.w;
        double p[3];
        d2d::move_point(T.m, (double)sp.x, (double)sp.y, (double)sp.z, p);
        // a row farther from the box of all finite target points than max_corr has no pair (as the ICP search leaves)
        const double ex = fmax(fmax(g.bx0 - p[0], p[0] - g.bx1), 0.0), ey = fmax(fmax(g.by0 - p[1], p[1] - g.by1), 0.0), ez = fmax(fmax(g.bz0 - p[2], p[2] - g.bz1), 0.0);
        if (d2d::finite(w) && (ex * ex + ey * ey + ez * ez) * 0.999999999 < max_corr2) {
            double A[6], S[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) A[k] = (double)A6[6 * i + k];
            d2d::rotate_cov(T.m, A, S);
            d2d::RowAcc acc;
            grid_box_walk(g, cellStart, icp_cell(p[0], g.ox, g.inv_c, g.gx), icp_cell(p[1], g.oy, g.inv_c, g.gy), icp_cell(p[2], g.oz, g.inv_c, g.gz), rings,
                          [&](int s0, int e0) {
                              for (int j = s0; j < e0; ++j) {
                                  const float4 q = Tq[j];
                                  const double r[3] = {p[0] - (double)q.x, p[1] - (double)q.y, p[2] - (double)q.z};
                                  const double d2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
                                  if (!(d2 < max_corr2)) continue;
                                  const float4 b0 = rec[2 * (int64_t)j], b1 = rec[2 * (int64_t)j + 1];
                                  const double v = (double)b1.z;
                                  if (!d2d::finite(v)) continue;
                                  const double B[6] = {(double)b0.x, (double)b0.y, (double)b0.z, (double)b0.w, (double)b1.x, (double)b1.y};
                                  double M[6], Mr[3], m;
                                  if (!d2d::pair_metric(S, B, s2, phi, r, M, Mr, &m)) { acc.singular += 1; continue; }
                                  d2d::row_add(acc, w * v, exp(-0.5 * m), M, Mr, m);
                              }
                          });
            d2d::row_expand(p, acc, out);
        }
    }
    block_fold_store<D2D_LEN, D2D_LEN, wave_sum_xor>(out, partials, (int)blockIdx.x);
}

}  // namespace gsr

using namespace gsr;

struct gsr_d2d_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    GridIndex index;                // the target's point grid (gsr_grid.h)
    DevBuf stage_xyz, stage_cov, stage_w, trec;                 // the target: staging of host arrays, the cell-ordered (B, v) records
    DevBuf raw_xyz, raw_cov, raw_w, src_order, src4, srcA;      // the source: as given (a copy), and in the order of the target's cells
    DevBuf partials, sums;
    bool have_target = false, have_source = false, src_weighted = false, src_sorted = false;
    int64_t nt = 0, ns = 0;
    double max_corr = 0;
    ~gsr_d2d_ctx() { (void)hipSetDevice(device); }
};

namespace {

int32_t sort_source(gsr_d2d_ctx* c) {
    if (c->src_sorted || !c->have_source || !c->have_target || c->ns == 0 || c->nt == 0) return GSR_OK;
    hipStream_t st = c->stream;
    const int64_t n = c->ns;
    GSR_TRY(c->src4.reserve((size_t)n * 16));
    GSR_TRY(c->srcA.reserve((size_t)n * 24));
    GSR_TRY(c->index.sort_by_cell(c->raw_xyz.as<float>(), n, c->src_order, st));
    hipLaunchKernelGGL(k_d2d_gather_source, dim3(stride_grid(n)), dim3(256), 0, st, n, c->src_order.as<unsigned>(), c->raw_xyz.as<float>(), c->raw_cov.as<float>(),
                       c->src_weighted ? c->raw_w.as<float>() : (const float*)nullptr, c->src4.as<float4>(), c->srcA.as<float>());
    GSR_HIP(hipGetLastError());
    GSR_HIP(hipStreamSynchronize(st));
    c->src_sorted = true;
    return GSR_OK;
}

// dT = the rigid update of xi = -H^-1 g (gsr_solve.h, rigid_from_euler6).  false: the solve gave something that is not finite (no update).
bool d2d_step(const double* s, double dT[16]) {
    double H[6][6], nb[6], x[6];
    sym6_from_upper(s, H);
    for (int a = 0; a < 6; ++a) nb[a] = -s[21 + a];
    solve6(H, nb, x);
    for (int a = 0; a < 6; ++a)
        if (!d2d::finite(x[a])) return false;
    rigid_from_euler6(x, dT);
    return true;
}

int32_t accumulate(gsr_d2d_ctx* c, const double* T, double cov_scale, double cov_floor, double* out, const char* who) {
    const char* why = d2d::check_scalars(T, cov_scale, cov_floor);
    if (why[0]) return fail(GSR_E_INVALID, "%s: %s", who, why);
    if (!out) return fail(GSR_E_INVALID, "%s: the output is NULL", who);
    if (!c) return fail(GSR_E_INVALID, "%s: NULL context", who);
    if (!c->have_target || !c->have_source) return fail(GSR_E_INVALID, "%s: target and source must be set first", who);
    for (int k = 0; k < D2D_LEN; ++k) out[k] = 0.0;
    if (c->ns == 0 || c->nt == 0) return GSR_OK;
    GSR_HIP(hipSetDevice(c->device));
    GSR_TRY(sort_source(c));
    hipStream_t st = c->stream;
    const int64_t nb64 = (c->ns + 255) / 256;
    const int nb = (int)nb64;
    GSR_TRY(c->partials.reserve((size_t)nb * D2D_LEN * 8));
    GSR_TRY(c->sums.reserve(D2D_LEN * 8));
    D2DXform X;
    for (int k = 0; k < 12; ++k) X.m[k] = T[k];
    const GridView gv = c->index.view();
    hipLaunchKernelGGL(k_d2d_accumulate, dim3(nb), dim3(256), 0, st, c->ns, c->src4.as<float4>(), c->srcA.as<float>(), X, cov_scale * cov_scale, cov_floor, gv.g,
                       gv.cellStart, gv.Tq, c->trec.as<float4>(), grid_rings_for_radius(gv.g, c->max_corr), c->max_corr * c->max_corr, c->partials.as<double>());
    hipLaunchKernelGGL(k_fold_partials<64>, dim3(D2D_LEN), dim3(64), 0, st, nb64, D2D_LEN, (const double*)c->partials.as<double>(), c->sums.as<double>());
    GSR_HIP(hipGetLastError());
    GSR_HIP(hipMemcpyAsync(out, c->sums.p, D2D_LEN * 8, hipMemcpyDeviceToHost, st));
    GSR_HIP(hipStreamSynchronize(st));
    return GSR_OK;
}

}  // namespace

extern "C" {

int32_t gsr_d2d_create(gsr_d2d_ctx** out, int32_t device, void* stream) {
    if (!out) return fail(GSR_E_INVALID, "gsr_d2d_create: out is NULL");
    *out = nullptr;
    GSR_TRY(open_device(device, "gsr_d2d_create"));
    gsr_d2d_ctx* c = new gsr_d2d_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;
    *out = c;
    return GSR_OK;
}

int32_t gsr_d2d_destroy(gsr_d2d_ctx* c) {
    delete c;       // (NULL: nothing)
    return GSR_OK;
}

int32_t gsr_d2d_set_target(gsr_d2d_ctx* c, const float* xyz, const float* cov6, const float* weight, int64_t n, double max_corr, int32_t on_device) {
    if (!(max_corr > 0) || !isfinite(max_corr)) return fail(GSR_E_INVALID, "gsr_d2d_set_target: max_corr must be positive and finite (got %g)", max_corr);
    if (n < 0) return fail(GSR_E_INVALID, "gsr_d2d_set_target: negative size (%lld)", (long long)n);
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "gsr_d2d_set_target: n too large");
    if (n > 0 && (!xyz || !cov6)) return fail(GSR_E_INVALID, "gsr_d2d_set_target: NULL points or covariances");
    if (!c) return fail(GSR_E_INVALID, "gsr_d2d_set_target: NULL context");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->have_target = false;
    c->src_sorted = false;              // the source is kept in the order of the target's cells
    if (n > 0) {
        const float *dx = xyz, *dc = cov6, *dw = weight;
        if (!on_device) {
            GSR_TRY(c->stage_xyz.reserve((size_t)n * 12));
            GSR_TRY(c->stage_cov.reserve((size_t)n * 24));
            GSR_HIP(hipMemcpyAsync(c->stage_xyz.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
            GSR_HIP(hipMemcpyAsync(c->stage_cov.p, cov6, (size_t)n * 24, hipMemcpyHostToDevice, st));
            dx = c->stage_xyz.as<float>();
            dc = c->stage_cov.as<float>();
            if (weight) {
                GSR_TRY(c->stage_w.reserve((size_t)n * 4));
                GSR_HIP(hipMemcpyAsync(c->stage_w.p, weight, (size_t)n * 4, hipMemcpyHostToDevice, st));
                dw = c->stage_w.as<float>();
            }
        }
        GSR_TRY(c->index.build(dx, n, max_corr, st));
        GSR_TRY(c->trec.reserve((size_t)n * 32));
        hipLaunchKernelGGL(k_d2d_gather_target, dim3(stride_grid(n)), dim3(256), 0, st, n, c->index.order.as<unsigned>(), dc, dw, c->trec.as<float4>());
        GSR_HIP(hipGetLastError());
        GSR_HIP(hipStreamSynchronize(st));
    }
    c->nt = n;
    c->max_corr = max_corr;
    c->have_target = true;
    return sort_source(c);
}

int32_t gsr_d2d_set_source(gsr_d2d_ctx* c, const float* xyz, const float* cov6, const float* weight, int64_t n, int32_t on_device) {
    if (n < 0) return fail(GSR_E_INVALID, "gsr_d2d_set_source: negative size (%lld)", (long long)n);
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "gsr_d2d_set_source: n too large");
    if (n > 0 && (!xyz || !cov6)) return fail(GSR_E_INVALID, "gsr_d2d_set_source: NULL points or covariances");
    if (!c) return fail(GSR_E_INVALID, "gsr_d2d_set_source: NULL context");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->have_source = false;
    c->src_sorted = false;
    if (n > 0) {
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        GSR_TRY(c->raw_xyz.reserve((size_t)n * 12));
        GSR_TRY(c->raw_cov.reserve((size_t)n * 24));
        GSR_HIP(hipMemcpyAsync(c->raw_xyz.p, xyz, (size_t)n * 12, kind, st));
        GSR_HIP(hipMemcpyAsync(c->raw_cov.p, cov6, (size_t)n * 24, kind, st));
        if (weight) {
            GSR_TRY(c->raw_w.reserve((size_t)n * 4));
            GSR_HIP(hipMemcpyAsync(c->raw_w.p, weight, (size_t)n * 4, kind, st));
        }
        GSR_HIP(hipStreamSynchronize(st));
    }
    c->src_weighted = n > 0 && weight != nullptr;
    c->ns = n;
    c->have_source = true;
    return sort_source(c);
}

int32_t gsr_d2d_accumulate(gsr_d2d_ctx* c, const double* T, double cov_scale, double cov_floor, double* out32) {
    return accumulate(c, T, cov_scale, cov_floor, out32, "gsr_d2d_accumulate");
}

int32_t gsr_d2d_register(gsr_d2d_ctx* c, const double* init_T, double cov_scale, double cov_floor, double relative_score, int32_t max_iter, double* out_T,
                         gsr_d2d_report* report) {
    const char* who = "gsr_d2d_register";
    const char* why = d2d::check_scalars(init_T, cov_scale, cov_floor);
    if (why[0]) return fail(GSR_E_INVALID, "%s: %s", who, why);
    if (!(relative_score >= 0) || !isfinite(relative_score)) return fail(GSR_E_INVALID, "%s: relative_score must be non-negative and finite", who);
    if (max_iter < 0) return fail(GSR_E_INVALID, "%s: negative max_iter (%d)", who, max_iter);
    if (!out_T || !report) return fail(GSR_E_INVALID, "%s: NULL output", who);
    if (!c) return fail(GSR_E_INVALID, "%s: NULL context", who);
    double T[16], s[D2D_LEN], prev = 0.0;
    for (int k = 0; k < 16; ++k) T[k] = init_T[k];
    int iterations = 0, status = GSR_D2D_MAX_ITERATION;
    bool have_prev = false;
    for (int it = 0;; ++it) {
        GSR_TRY(accumulate(c, T, cov_scale, cov_floor, s, who));                // (after the last step too: the report is at the final T)
        if (s[d2d::S_PAIRS] == 0.0) { status = GSR_D2D_NO_PAIRS; break; }
        if (have_prev && fabs(s[d2d::S_SCORE] - prev) <= relative_score * s[d2d::S_SCORE]) { status = GSR_D2D_CONVERGED; break; }
        if (it >= max_iter) break;
        double dT[16];
        if (!d2d_step(s, dT)) { status = GSR_D2D_DEGENERATE; break; }
        mat4_mul(dT, T, T);
        prev = s[d2d::S_SCORE];
        have_prev = true;
        ++iterations;
    }
    for (int k = 0; k < 16; ++k) out_T[k] = T[k];
    report->score = s[d2d::S_SCORE];
    report->fitness = c->ns > 0 ? s[d2d::S_ROWS] / (double)c->ns : 0.0;
    report->mahalanobis_rmse = s[d2d::S_SCORE] > 0 ? sqrt(s[d2d::S_WM] / s[d2d::S_SCORE]) : 0.0;
    report->n_pairs = (int64_t)s[d2d::S_PAIRS];
    report->n_singular = (int64_t)s[d2d::S_SINGULAR];
    report->iterations = iterations;
    report->status = status;
    return GSR_OK;
}

}  // extern "C"
