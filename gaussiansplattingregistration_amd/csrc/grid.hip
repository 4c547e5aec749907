// grid.hip -- the point grid (gsr_grid.h; DESIGN.md, "the point grid"): GridIndex builds the cell-sorted uniform grid over a cloud,
// and the two stateless searches that need nothing but that grid live here with it.
//
//   GridIndex::build        k_icp_bbox / _reduce, k_icp_hist + k_icp_trim (the robust box, once or twice), the cell size on the host,
//                           k_icp_keys, rocPRIM sort by cell, k_icp_cell_starts, k_icp_gather_target
//   GridIndex::sort_by_cell k_icp_keys + the sort, for another cloud over the same cells (the ICP source)
//   GridIndex::fetch        k_icp_publish into pinned memory the host polls
//   gsr_normals_knn         k_knn_normals: a thread per point, grid_ring_walk into a KBest list
//   hybrid_search_dev       k_hybrid_search: a wave per point, grid_box_walk + wave_scan_take, the output ranked by hyb_rank_cut
#include "gsr_grid.h"
#include "gsr_normals.h"
#include "gsr_oneshot.h"
#include "gsr_prims.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace gsr {
// rocPRIM's Onesweep with its gfx950 kernel shapes but 11 bits per pass: the 22-bit cell keys of a 5 M-point grid take two passes
// instead of three (up to 2^20 keys rocPRIM's merge sort runs as before)
// (the merge sorts of up to 2^20 keys with block sorts of 1 024 x 4 keys: 20-25 us less per target / source sort at 556 k points than rocPRIM's
// default shape, equal at 185 k: profiles/r05aj_icp_merge_sort_configs.txt)
#ifndef GSR_ICP_MERGE_BS
#define GSR_ICP_MERGE_BS 1024
#define GSR_ICP_MERGE_IPT 4
#endif
using icp_merge_cfg = rocprim::merge_sort_config<512, GSR_ICP_MERGE_BS, GSR_ICP_MERGE_IPT, 128, 128, 4>;
using icp_sort_cfg = rocprim::radix_sort_config<rocprim::default_config, icp_merge_cfg,
                                                rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 16>, rocprim::kernel_config<1024, 16>, 11,
                                                                                    rocprim::block_radix_rank_algorithm::match>>;

#ifndef ICP_CELL_FLOOR_DIV
#define ICP_CELL_FLOOR_DIV 64.0     // a grid cell is never finer than max_corr / this (bounds the rings of a query that finds nothing)
#endif
__global__ __launch_bounds__(256) void k_icp_bbox(int64_t n, const float* __restrict__ xyz, float* __restrict__ bbox_part) {
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX) {
            mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
            mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
            mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
        }
    }
    // per-block partial box, no atomics (10^4 same-address atomics cost ~0.5 ms: they serialise across the XCDs)
    __shared__ float s_mn[4][3], s_mx[4][3];
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) { s_mn[threadIdx.x >> 6][k] = mn[k]; s_mx[threadIdx.x >> 6][k] = mx[k]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        float a = s_mn[0][k], b = s_mx[0][k];
        for (int w = 1; w < 4; ++w) { a = fminf(a, s_mn[w][k]); b = fmaxf(b, s_mx[w][k]); }
        bbox_part[6 * blockIdx.x + k] = a;
        bbox_part[6 * blockIdx.x + 3 + k] = b;
    }
}
// bbox[0..2] = min, bbox[3..5] = max over the per-block partial boxes
__global__ __launch_bounds__(256) void k_icp_bbox_reduce(int nblocks, const float* __restrict__ part, float* __restrict__ bbox) {
    __shared__ float s_v[4][6];
    float v[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
        for (int k = 0; k < 3; ++k) { v[k] = fminf(v[k], part[6 * b + k]); v[3 + k] = fmaxf(v[3 + k], part[6 * b + 3 + k]); }
    for (int k = 0; k < 3; ++k)
        for (int o = 32; o > 0; o >>= 1) { v[k] = fminf(v[k], __shfl_xor(v[k], o)); v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], o)); }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; ++k) s_v[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        float r = s_v[0][k];
        for (int w = 1; w < 4; ++w) r = k < 3 ? fminf(r, s_v[w][k]) : fmaxf(r, s_v[w][k]);
        bbox[k] = r;
    }
}

// A robust box for the grid.  The reference's scenes come with floaters: a dozen points at 50 scene radii make the box of ALL points
// 10^5 times the scene's volume, the cells -- sized for two points each over that box -- swallow the scene whole, and every query
// scans millions of points (found with bench.py --workload clustered: 116 s per registration).  So: per-axis histograms over the raw
// box (ICP_HIST_BINS bins), the range that holds all but the outermost 0.1 % of the points per side; when that range is less than
// half the raw extent on some axis the grid is laid over it (after ONE refinement pass at the finer resolution), and the points
// beyond are clamped into the boundary cells, which every search treats as half-infinite (icp_slab_dist; the ring logic skips the
// boundary faces anyway).  A cloud without outliers keeps the raw box: nothing changes for it.
#define ICP_HIST_BINS 1024
__global__ __launch_bounds__(256) void k_icp_hist(int64_t n, const float* __restrict__ xyz, const float* __restrict__ box, unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[3 * ICP_HIST_BINS];
    for (int k = threadIdx.x; k < 3 * ICP_HIST_BINS; k += blockDim.x) s_h[k] = 0u;
    __syncthreads();
    float mn[3], sc[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = box[k];
        const float ext = box[3 + k] - mn[k];
        sc[k] = ext > 0.0f ? (float)ICP_HIST_BINS / ext : 0.0f;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (fabsf(v[0]) <= FLT_MAX && fabsf(v[1]) <= FLT_MAX && fabsf(v[2]) <= FLT_MAX) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float t = (v[k] - mn[k]) * sc[k];
                t = fminf(fmaxf(t, 0.0f), (float)(ICP_HIST_BINS - 1));
                atomicAdd(&s_h[k * ICP_HIST_BINS + (int)t], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * ICP_HIST_BINS; k += blockDim.x)
        if (s_h[k]) atomicAdd(&hist[k], s_h[k]);
}
// box_out = per axis the bins [lo, hi] of box_in that hold all but the outermost 0.1 % of the points per side, widened by one bin on
// either side; *flag = 1 when on some axis that is less than half of box_in's extent.  One thread per axis.
__global__ void k_icp_trim(const unsigned* __restrict__ hist, const float* __restrict__ box_in, float* __restrict__ box_out, float* __restrict__ flag) {
    __shared__ int s_narrow[3];
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const unsigned* h = hist + k * ICP_HIST_BINS;
        unsigned long long total = 0;
        for (int b = 0; b < ICP_HIST_BINS; ++b) total += h[b];
        const unsigned long long trim = total / 1000ull;
        int lo = 0, hi = ICP_HIST_BINS - 1;
        unsigned long long acc = 0;
        while (lo < ICP_HIST_BINS - 1 && acc + h[lo] <= trim) { acc += h[lo]; ++lo; }
        acc = 0;
        while (hi > lo && acc + h[hi] <= trim) { acc += h[hi]; --hi; }
        const float mn = box_in[k], ext = box_in[3 + k] - mn, w = ext / (float)ICP_HIST_BINS;
        lo = lo > 0 ? lo - 1 : 0;
        hi = hi < ICP_HIST_BINS - 1 ? hi + 1 : ICP_HIST_BINS - 1;
        box_out[k] = mn + (float)lo * w;
        box_out[3 + k] = mn + (float)(hi + 1) * w;
        s_narrow[k] = (float)(hi + 1 - lo) * w < 0.5f * ext ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) *flag = (s_narrow[0] | s_narrow[1] | s_narrow[2]) ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void k_icp_keys(int64_t n, const float* __restrict__ xyz, IcpGrid g,
                                                  unsigned* __restrict__ keys, unsigned* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int cx = icp_cell((double)xyz[3 * i], g.ox, g.inv_c, g.gx);
        int cy = icp_cell((double)xyz[3 * i + 1], g.oy, g.inv_c, g.gy);
        int cz = icp_cell((double)xyz[3 * i + 2], g.oz, g.inv_c, g.gz);
        keys[i] = (unsigned)((cz * g.gy + cy) * g.gx + cx);
        idx[i] = (unsigned)i;
    }
}

__global__ __launch_bounds__(256) void k_icp_cell_starts(int64_t m, const unsigned* __restrict__ skeys, int64_t nkeys,
                                                         int* __restrict__ start) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        unsigned k = skeys[j];
        int64_t prev = j == 0 ? -1 : (int64_t)skeys[j - 1];
        if ((int64_t)k != prev)
            for (int64_t c = prev + 1; c <= (int64_t)k; ++c) start[c] = (int)j;
        if (j == m - 1)
            for (int64_t c = (int64_t)k + 1; c <= nkeys; ++c) start[c] = (int)m;
    }
}

__global__ __launch_bounds__(256) void k_icp_gather_target(int64_t n, const unsigned* __restrict__ order,
                                                           const float* __restrict__ xyz, const double* __restrict__ nrm,
                                                           float4* __restrict__ Tq, double* __restrict__ Tn) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned i = order[j];
        Tq[j] = make_float4(xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1], xyz[3 * (int64_t)i + 2], __uint_as_float(i));
        if (nrm) {
            Tn[3 * j] = nrm[3 * (int64_t)i]; Tn[3 * j + 1] = nrm[3 * (int64_t)i + 1]; Tn[3 * j + 2] = nrm[3 * (int64_t)i + 2];
        }
    }
}

// Normals of a cloud WITHOUT covariances: Open3D EstimateNormals(KDTreeSearchParamKNN(knn)) -- what the reference does to a
// sparse input cloud (src/utils/point_cloud_converter.py:9-28, default knn = 30).  One thread per point: its knn nearest
// points (itself included) by (distance, input index); with >= 3 of them the covariance by cumulants (Open3D ComputeCovariance),
// else the identity; normal_of_cov_d.  Output in the CALLER's point order (order[j] = input index of sorted point j).
__global__ __launch_bounds__(256) void k_knn_normals(int64_t nt, IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq,
                                                     const unsigned* __restrict__ order, int knn, double* __restrict__ out) {
    for (int64_t jq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; jq < nt; jq += (int64_t)gridDim.x * blockDim.x) {
        const float4 qv = Tq[jq];
        const double px = (double)qv.x, py = (double)qv.y, pz = (double)qv.z;
        double* o = out + 3 * (int64_t)order[jq];
        o[0] = 0.0; o[1] = 0.0; o[2] = 1.0;
        if (!(px == px) || !(py == py) || !(pz == pz)) continue;
        KBest<ICP_KNN> kb;
        const int rmax = (g.gx > g.gy ? g.gx : g.gy) > g.gz ? (g.gx > g.gy ? g.gx : g.gy) : g.gz;
        grid_ring_walk(g, cellStart, Tq, px, py, pz, rmax,
                       [&](int j, const float4& q, double d2) { if (d2 == d2) kb.offer(knn, d2, j, __float_as_uint(q.w)); },
                       [&](double reach2) { return kb.closed(knn, reach2); });
        const int cnt = kb.cnt;
        const int* kj = kb.j;
        double c00 = 1, c01 = 0, c02 = 0, c11 = 1, c12 = 0, c22 = 1;        // fewer than 3 neighbours: identity
        if (cnt >= 3) {
            double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = 0; i < cnt; ++i) {
                const float4 q = Tq[kj[i]];
                const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
                m[0] += x; m[1] += y; m[2] += z;
                m[3] += x * x; m[4] += x * y; m[5] += x * z; m[6] += y * y; m[7] += y * z; m[8] += z * z;
            }
            for (int k = 0; k < 9; ++k) m[k] /= (double)cnt;
            c00 = m[3] - m[0] * m[0]; c11 = m[6] - m[1] * m[1]; c22 = m[8] - m[2] * m[2];
            c01 = m[4] - m[0] * m[1]; c02 = m[5] - m[0] * m[2]; c12 = m[7] - m[1] * m[2];
        }
        double v[3];
        normal_of_cov_d(c00, c01, c02, c11, c12, c22, v);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" {
// Small device results the host waits for (the bounding box, the loop state) are copied by one tiny kernel into pinned host
// memory, the sequence number of the round trip last, and the host polls that word: a hipMemcpyAsync into pageable memory
// plus hipStreamSynchronize costs 30-50 us per round trip (wait_host_flag, gsr_common.h: the HEM read-backs wait the same way).
__global__ void k_icp_publish(const unsigned* __restrict__ src, int nwords, unsigned* __restrict__ host, unsigned long long* __restrict__ flag,
                              unsigned long long seq) {
    for (int t = threadIdx.x; t < nwords; t += blockDim.x) __hip_atomic_store(host + t, src[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // extern "C"

GridIndex::GridIndex() {
    if (const char* e = getenv("GSR_ICP_ROBUST_BOX")) robust_allowed = atoi(e) != 0;
    if (const char* e = getenv("GSR_ICP_CELL_TARGET")) { double v = atof(e); if (v > 0.01 && v < 1000) cell_target = v; }
    if (const char* e = getenv("GSR_ICP_MAX_CELLS")) { int v = atoi(e); if (v >= 1024) max_cells = v; }
    // pinned, device-mapped, COHERENT host memory: the device's system-scope stores must reach the host while the stream is still
    // running (a non-coherent mapping would only show them at the end of the kernel).  GSR_ICP_RB_POLL=0: no polling at all
    bool poll = true;
    if (const char* e = getenv("GSR_ICP_RB_POLL")) poll = atoi(e) != 0;
    if (!poll || host_rb.alloc(1024 + 64) != hipSuccess) (void)hipGetLastError();
}

int32_t GridIndex::fetch(hipStream_t st, const void* dev, void* out, size_t bytes) {
    unsigned* const rb = host_rb.as<unsigned>();
    if (!rb || bytes > 1024 || (bytes & 3)) {
        GSR_HIP(hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, st));
        GSR_HIP(hipStreamSynchronize(st));
        return GSR_OK;
    }
    const unsigned long long seq = ++rb_seq;
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(rb + 256);
    hipLaunchKernelGGL(k_icp_publish, dim3(1), dim3(64), 0, st, (const unsigned*)dev, (int)(bytes >> 2), rb, flag, seq);
    GSR_HIP(hipGetLastError());
    GSR_TRY(wait_host_flag(st, flag, seq, true));       // (GSR_ICP_RB_POLL=0 left host_rb empty: the copy above)
    memcpy(out, (const void*)rb, bytes);
    return GSR_OK;
}

int32_t GridIndex::sort_by_cell(const float* xyz_dev, int64_t n_pts, DevBuf& order_out, hipStream_t st) {
    GSR_TRY(keys.reserve(n_pts * 4)); GSR_TRY(idx.reserve(n_pts * 4)); GSR_TRY(skeys.reserve(n_pts * 4)); GSR_TRY(order_out.reserve(n_pts * 4));
    hipLaunchKernelGGL(k_icp_keys, dim3(stride_grid(n_pts)), dim3(256), 0, st, n_pts, xyz_dev, grid, keys.as<unsigned>(), idx.as<unsigned>());
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < grid.ncells) ++bits;
    return sort_pairs_by_key<icp_sort_cfg>(rocprim_tmp, st, keys.as<unsigned>(), skeys.as<unsigned>(), idx.as<unsigned>(), order_out.as<unsigned>(),
                                           (size_t)n_pts, 0u, (unsigned)bits);
}

int32_t GridIndex::build(const float* dxyz, int64_t n, double max_corr, hipStream_t st, const double* dnrm, double* Tn) {
    if (!(max_corr > 0)) return fail(GSR_E_PRECONDITION, "max_correspondence_distance must be > 0 (got %g)", max_corr);
    if (n <= 0 || !dxyz) return fail(GSR_E_PRECONDITION, "point grid: empty cloud");
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "point grid: n too large");
    // bounding box of the finite points
    const int nbb = stride_grid(n);
    GSR_TRY(bbox.reserve(64 + (size_t)nbb * 24));
    hipLaunchKernelGGL(k_icp_bbox, dim3(nbb), dim3(256), 0, st, n, dxyz, bbox.as<float>() + 16);
    hipLaunchKernelGGL(k_icp_bbox_reduce, dim3(1), dim3(256), 0, st, nbb, bbox.as<float>() + 16, bbox.as<float>());
    // the robust candidate of the raw box: header floats [0..5] raw, [6..11] trimmed, [12] "the raw box is far too large"
    GSR_TRY(hist.reserve(3 * ICP_HIST_BINS * 4));
    GSR_HIP(hipMemsetAsync(hist.p, 0, 3 * ICP_HIST_BINS * 4, st));
    hipLaunchKernelGGL(k_icp_hist, dim3(nbb > 512 ? 512 : nbb), dim3(256), 0, st, n, dxyz, bbox.as<float>(), hist.as<unsigned>());
    hipLaunchKernelGGL(k_icp_trim, dim3(1), dim3(64), 0, st, hist.as<unsigned>(), bbox.as<float>(), bbox.as<float>() + 6, bbox.as<float>() + 12);
    float hb[13];
    GSR_TRY(fetch(st, bbox.p, hb, 13 * 4));
    const float raw_box[6] = {hb[0], hb[1], hb[2], hb[3], hb[4], hb[5]};
    robust_box = hb[12] != 0.0f && robust_allowed;
    if (robust_box) {        // far outliers: one refinement at the resolution of the trimmed range, then the grid goes over THAT
        GSR_HIP(hipMemsetAsync(hist.p, 0, 3 * ICP_HIST_BINS * 4, st));
        hipLaunchKernelGGL(k_icp_hist, dim3(nbb > 512 ? 512 : nbb), dim3(256), 0, st, n, dxyz, bbox.as<float>() + 6, hist.as<unsigned>());
        hipLaunchKernelGGL(k_icp_trim, dim3(1), dim3(64), 0, st, hist.as<unsigned>(), bbox.as<float>() + 6, bbox.as<float>(), bbox.as<float>() + 12);
        GSR_TRY(fetch(st, bbox.p, hb, 6 * 4));
    }
    double mn[3], mx[3];
    for (int k = 0; k < 3; ++k) { mn[k] = hb[k]; mx[k] = hb[3 + k]; }
    IcpGrid g;
    if (!(mx[0] >= mn[0])) { mn[0] = mn[1] = mn[2] = 0; mx[0] = mx[1] = mx[2] = 0; }
    // cell: about two target points per cell, but no finer than max_corr/8 (bounds the ring count)
    double cell;
    {
        const double ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
        const double emax = fmax(ex, fmax(ey, ez)), eps = emax * 1e-6 + 1e-30;
        cell = cbrt((ex + eps) * (ey + eps) * (ez + eps) * cell_target / (double)n);
        if (!(cell > 0)) cell = max_corr;
        // (round 6: max_corr / 64, was / 8.  The floor bounds the ring count of a query that finds nothing; with / 8 the reference's DEFAULT
        // max_correspondence of 5 scene units put 450 points into every cell of a 1 M-splat cloud and an iteration took 4.9 ms instead of
        // 0.15, scripts/icp_default_params.py.  A query beyond the target's box + max_corr leaves before the first ring, icp_nearest)
        if (cell < max_corr / ICP_CELL_FLOOR_DIV) cell = max_corr / ICP_CELL_FLOOR_DIV;
    }
    for (;;) {
        double fx = floor((mx[0] - mn[0]) / cell) + 1, fy = floor((mx[1] - mn[1]) / cell) + 1, fz = floor((mx[2] - mn[2]) / cell) + 1;
        if (fx * fy * fz <= (double)max_cells) { g.gx = (int)fx; g.gy = (int)fy; g.gz = (int)fz; break; }
        cell *= 1.2599210498948732;
    }
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
    g.c = cell; g.inv_c = 1.0 / cell;
    g.cx = 0.5 * (mn[0] + mx[0]); g.cy = 0.5 * (mn[1] + mx[1]); g.cz = 0.5 * (mn[2] + mx[2]);
    g.ncells = g.gx * g.gy * g.gz;
    g.rings = (int)ceil(max_corr / cell);
    if (g.rings < 1) g.rings = 1;
    g.bx0 = raw_box[0]; g.by0 = raw_box[1]; g.bz0 = raw_box[2]; g.bx1 = raw_box[3]; g.by1 = raw_box[4]; g.bz1 = raw_box[5];
    if (!(raw_box[3] >= raw_box[0])) { g.bx0 = g.by0 = g.bz0 = -1.0 / 0.0; g.bx1 = g.by1 = g.bz1 = 1.0 / 0.0; }      // (no finite point: no box, no early leave)
    grid = g;
    this->n = n;
    GSR_TRY(sort_by_cell(dxyz, n, order, st));
    GSR_TRY(cellStart.reserve(((size_t)g.ncells + 1) * 4));
    hipLaunchKernelGGL(k_icp_cell_starts, dim3(stride_grid(n)), dim3(256), 0, st, n, skeys.as<unsigned>(), (int64_t)g.ncells, cellStart.as<int>());
    GSR_TRY(Tq.reserve((size_t)n * 16));
    hipLaunchKernelGGL(k_icp_gather_target, dim3(stride_grid(n)), dim3(256), 0, st, n, order.as<unsigned>(), dxyz, dnrm, Tq.as<float4>(), dnrm ? Tn : (double*)nullptr);
    GSR_HIP(hipGetLastError());                      // the launches of the index build
    return GSR_OK;
}

extern "C" int32_t gsr_normals_knn(const float* xyz, int64_t n, int32_t knn, double* normals, int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!xyz || !normals))) return fail(GSR_E_INVALID, "gsr_normals_knn: bad argument");
    if (knn < 1 || knn > ICP_KNN) return fail(GSR_E_INVALID, "gsr_normals_knn: knn must lie in [1, %d] (got %d)", ICP_KNN, knn);
    if (n == 0) return GSR_OK;
    GSR_TRY(open_device(device, "gsr_normals_knn"));
    GridIndex gi;                                    // before the OneShot: it waits before the grid's buffers are freed
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_normals_knn");
    const float* dxyz = nullptr;
    double* out = nullptr;
    GSR_TRY(os.in(xyz, (size_t)n * 12, &dxyz));
    GSR_TRY(os.out(normals, (size_t)n * 24, &out));
    GSR_TRY(gi.build(dxyz, n, 1e-300, os.st));       // about two points per cell; a correspondence distance plays no role here
    hipLaunchKernelGGL(k_knn_normals, dim3(stride_grid(n)), dim3(256), 0, os.st, n, gi.grid, gi.cellStart.as<int>(), gi.Tq.as<float4>(), gi.order.as<unsigned>(),
                       (int)knn, out);
    return os.finish();
}

// ---- hybrid radius / count search (FPFH neighbourhoods, csrc/features.hip) ------------------------------------------------
// One wave per query point over the grid of the cloud itself: every cell within ceil(radius / cell) + 1 rings is read as contiguous row
// spans, the lanes test d^2 <= radius^2 and append the hits to an LDS list by ballot.  When the list would overflow it is cut to the
// max_nn best by rank (keys (d^2, index) are unique), and from then on only candidates ahead of the max_nn-th key are taken.  At the
// end each entry's rank among the list is its slot: the output is sorted by (d^2, index) without a sort.
namespace gsr {

__global__ __launch_bounds__(64) void k_hybrid_search(int64_t n, IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq,
                                                      double r2, int R, int max_nn, int* __restrict__ nbr, int* __restrict__ cnt_out) {
    __shared__ double sd[GSR_HYBRID_CAP];
    __shared__ unsigned si[GSR_HYBRID_CAP];
    const int lane = threadIdx.x;
    for (int64_t jq = blockIdx.x; jq < n; jq += gridDim.x) {
        const float4 qv = Tq[jq];
        const int64_t row = (int64_t)__float_as_uint(qv.w);          // input index of the query
        const double px = (double)qv.x, py = (double)qv.y, pz = (double)qv.z;
        int cnt = 0;
        bool pruned = false;
        double thr_d = 0.0;
        unsigned thr_i = 0u;
        if (px == px && py == py && pz == pz)
            grid_box_walk(g, cellStart, icp_cell(px, g.ox, g.inv_c, g.gx), icp_cell(py, g.oy, g.inv_c, g.gy), icp_cell(pz, g.oz, g.inv_c, g.gz), R, [&](int s0, int e0) {
                wave_scan_take(Tq, s0, e0, px, py, pz, sd, si, cnt, max_nn,
                               [&](double d2, unsigned qi) { return d2 <= r2 && (!pruned || hyb_less(d2, qi, thr_d, thr_i)); },
                               [&]() { pruned = true; thr_d = sd[max_nn - 1]; thr_i = si[max_nn - 1]; });
            });
        const int keep = cnt < max_nn ? cnt : max_nn;
        hyb_rank_cut(sd, si, cnt, max_nn, nbr + row * max_nn);
        if (lane == 0) cnt_out[row] = keep;
        __syncthreads();
    }
}

int32_t hybrid_search_dev(const float* xyz_dev, int64_t n, double radius, int max_nn, int device, hipStream_t stream, int* nbr_dev, int* cnt_dev) {
    if (n <= 0) return GSR_OK;
    GSR_HIP(hipSetDevice(device));
    GridIndex gi;
    GSR_TRY(gi.build(xyz_dev, n, radius, stream));                     // about two points per cell, no finer than radius / 64
    const int blocks = n < 16384 ? (int)n : 16384;
    hipLaunchKernelGGL(k_hybrid_search, dim3(blocks), dim3(64), 0, stream, n, gi.grid, gi.cellStart.as<int>(), gi.Tq.as<float4>(), radius * radius,
                       grid_rings_for_radius(gi.grid, radius), max_nn, nbr_dev, cnt_dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);             // (before the grid's buffers are freed)
    if (e != hipSuccess) return fail(GSR_E_HIP, "hybrid search: %s", hipGetErrorString(e));
    return GSR_OK;
}

}  // namespace gsr
