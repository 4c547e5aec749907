// gsr_fuse_dev.h -- what the pairwise overlap merge (fuse.hip) and the N-way one (fuse_multi.hip) share: the per-row pre-pass, the robust
// box and the grid over the valid centres, the cell keys and starts with the host code that launches them (FuseCells), and the two
// forms of the symmetrised KL divergence.  The kernels are `static`: each translation unit that includes this gets its own copy.
#pragma once
#include "gsr_common.h"
#include "gsr_oneshot.h"
#include "gsr_prims.h"

#include <float.h>
#include <math.h>

namespace gsr {

struct FuseGrid {
    double ox, oy, oz, inv_c;
    int gx, gy, gz, ncells;
};
#define FUSE_MOM 13      // count, sum x y z, sum xx yy zz, min x y z, max x y z

__device__ __forceinline__ int fuse_cell(double v, double o, double inv_c, int g) {
    double t = (v - o) * inv_c;
    t = fmin(fmax(t, 0.0), (double)(g - 1));      // NaN -> 0
    return (int)t;
}

// validity, weight and inverse covariance of every splat; counts the invalid ones (one atomic per wave that has any)
static __global__ __launch_bounds__(256) void k_fuse_prep(int64_t n, const float* __restrict__ xyz, const float* __restrict__ cov6, const float* __restrict__ opacity,
                                                   double* __restrict__ w, double* __restrict__ inv, unsigned long long* __restrict__ n_invalid) {
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < n;
        bool valid = false;
        if (live) {
            const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2], op = opacity[i];
            const double c00 = cov6[6 * i], c01 = cov6[6 * i + 1], c02 = cov6[6 * i + 2], c11 = cov6[6 * i + 3], c12 = cov6[6 * i + 4], c22 = cov6[6 * i + 5];
            const double m00 = c11 * c22 - c12 * c12, m01 = c02 * c12 - c01 * c22, m02 = c01 * c12 - c02 * c11;
            const double det = c00 * m00 + c01 * m01 + c02 * m02;
            double wi = 0.0;
            if (fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX && fabs(op) <= DBL_MAX && fabs(c00) <= DBL_MAX && fabs(c01) <= DBL_MAX &&
                fabs(c02) <= DBL_MAX && fabs(c11) <= DBL_MAX && fabs(c12) <= DBL_MAX && fabs(c22) <= DBL_MAX && det > 0.0) {      // (NaN fails every test)
                wi = (1.0 / (1.0 + exp(-op))) * sqrt(det);
                if (!(wi > 0.0 && wi <= DBL_MAX)) wi = 0.0;
            }
            valid = wi > 0.0;
            w[i] = wi;
            const double m11 = c00 * c22 - c02 * c02, m12 = c01 * c02 - c00 * c12, m22 = c00 * c11 - c01 * c01;
            double* o = inv + 6 * i;
            if (valid) { o[0] = m00 / det; o[1] = m01 / det; o[2] = m02 / det; o[3] = m11 / det; o[4] = m12 / det; o[5] = m22 / det; }
            else { o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0; }
        }
        const unsigned long long m = __ballot(live && !valid);
        if (m != 0ull && lane == 0) atomicAdd(n_invalid, (unsigned long long)__popcll(m));
    }
}

// per-block moments of the valid centres (inside `box` when given): FUSE_MOM doubles per block, fixed order, no atomics
static __global__ __launch_bounds__(256) void k_fuse_moments(int64_t n, const float* __restrict__ xyz, const double* __restrict__ w, const double* __restrict__ box,
                                                      double* __restrict__ part) {
    double a[FUSE_MOM];
    for (int k = 0; k < 7; ++k) a[k] = 0.0;
    for (int k = 0; k < 3; ++k) { a[7 + k] = DBL_MAX; a[10 + k] = -DBL_MAX; }
    double lo[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX}, hi[3] = {DBL_MAX, DBL_MAX, DBL_MAX};
    if (box) for (int k = 0; k < 3; ++k) { lo[k] = box[k]; hi[k] = box[3 + k]; }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!(w[i] > 0.0)) continue;
        const double p[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        if (!(p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2])) continue;
        a[0] += 1.0;
        for (int k = 0; k < 3; ++k) { a[1 + k] += p[k]; a[4 + k] += p[k] * p[k]; a[7 + k] = fmin(a[7 + k], p[k]); a[10 + k] = fmax(a[10 + k], p[k]); }
    }
    __shared__ double s[4][FUSE_MOM];
    for (int k = 0; k < FUSE_MOM; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            const double v = __shfl_xor(a[k], o);
            a[k] = k < 7 ? a[k] + v : k < 10 ? fmin(a[k], v) : fmax(a[k], v);
        }
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < FUSE_MOM; ++k) s[threadIdx.x >> 6][k] = a[k];
    __syncthreads();
    if (threadIdx.x < FUSE_MOM) {
        const int k = threadIdx.x;
        double v = s[0][k];
        for (int j = 1; j < 4; ++j) v = k < 7 ? v + s[j][k] : k < 10 ? fmin(v, s[j][k]) : fmax(v, s[j][k]);
        part[(int64_t)blockIdx.x * FUSE_MOM + k] = v;
    }
}

// one block: the partial moments summed in block order; stage 0 writes the 3-sigma box of the first pass to box[0..5], stage 1
// the grid.  Edge = max_distance (1 + 1e-6) -- the margin keeps the rounding of (v - o) * inv_c from separating two centres that
// are exactly max_distance apart by two cells -- times 2^(1/3) until gx gy gz <= cap.
static __global__ __launch_bounds__(64) void k_fuse_box(int nblocks, const double* __restrict__ part, int stage, double max_distance, int64_t cap,
                                                 double* __restrict__ box, FuseGrid* __restrict__ grid) {
    __shared__ double m[FUSE_MOM];
    if (threadIdx.x < FUSE_MOM) {
        const int k = threadIdx.x;
        double v = part[k];
        for (int b = 1; b < nblocks; ++b) { const double u = part[(int64_t)b * FUSE_MOM + k]; v = k < 7 ? v + u : k < 10 ? fmin(v, u) : fmax(v, u); }
        m[k] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (m[0] > 0.0) {
        const double f = stage == 0 ? 3.0 : 4.0;
        for (int k = 0; k < 3; ++k) {
            const double mean = m[1 + k] / m[0];
            double var = m[4 + k] / m[0] - mean * mean;
            if (!(var > 0.0)) var = 0.0;
            const double sd = sqrt(var);
            lo[k] = fmax(mean - f * sd, m[7 + k]);
            hi[k] = fmin(mean + f * sd, m[10 + k]);
            if (!(hi[k] >= lo[k])) { lo[k] = m[7 + k]; hi[k] = m[10 + k]; }
        }
    }
    if (stage == 0) {
        for (int k = 0; k < 3; ++k) { box[k] = lo[k]; box[3 + k] = hi[k]; }
        return;
    }
    FuseGrid g;
    g.ox = lo[0]; g.oy = lo[1]; g.oz = lo[2];
    double cell = max_distance * (1.0 + 1e-6);
    g.gx = g.gy = g.gz = 1;
    g.inv_c = 0.0;
    for (int it = 0; it < 8192; ++it) {
        const double fx = floor((hi[0] - lo[0]) / cell) + 1.0, fy = floor((hi[1] - lo[1]) / cell) + 1.0, fz = floor((hi[2] - lo[2]) / cell) + 1.0;
        if (fx * fy * fz <= (double)cap) { g.gx = (int)fx; g.gy = (int)fy; g.gz = (int)fz; g.inv_c = 1.0 / cell; break; }
        cell *= 1.2599210498948732;
    }
    g.ncells = g.gx * g.gy * g.gz;
    *grid = g;
}

static __global__ __launch_bounds__(256) void k_fuse_keys(int64_t n, const float* __restrict__ xyz, const FuseGrid* __restrict__ G, unsigned* __restrict__ keys,
                                                   unsigned* __restrict__ idx) {
    const FuseGrid g = *G;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int cx = fuse_cell(xyz[3 * i], g.ox, g.inv_c, g.gx), cy = fuse_cell(xyz[3 * i + 1], g.oy, g.inv_c, g.gy), cz = fuse_cell(xyz[3 * i + 2], g.oz, g.inv_c, g.gz);
        keys[i] = (unsigned)((cz * g.gy + cy) * g.gx + cx);
        idx[i] = (unsigned)i;
    }
}

// start[c] = the first position of the sorted keys that is >= c, for c = 0 .. cap (every entry is written: the cell count lives on the device)
static __global__ __launch_bounds__(256) void k_fuse_cell_starts(int64_t n, const unsigned* __restrict__ skeys, int64_t cap, int* __restrict__ start) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= cap; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)skeys[mid] < c) lo = mid + 1; else hi = mid;
        }
        start[c] = (int)lo;
    }
}

// tr(P Q) of two symmetric 3x3 in the six-entry form (xx, xy, xz, yy, yz, zz)
__device__ __forceinline__ double sym_trace(const double* P, const double* Q) {
    return ((P[0] * Q[0] + P[3] * Q[3]) + P[5] * Q[5]) + 2.0 * ((P[1] * Q[1] + P[2] * Q[2]) + P[4] * Q[4]);
}
__device__ __forceinline__ double sym_quad(const double* P, double x, double y, double z) {
    return ((P[0] * x * x + P[3] * y * y) + P[5] * z * z) + 2.0 * ((P[1] * x * y + P[2] * x * z) + P[4] * y * z);
}

// The front both merges share, for the `n` rows the grid is built over (all of A, or the union): k_fuse_prep into w / inv (n_invalid
// zeroed by the caller), the robust box over the valid centres, the table of at most `cap` = max(n, 1024) cells, the rows in cell order
// and the cell starts.  reserve() asks for the device memory (added to `workspace`; rocPRIM's stays in tmp_sort) and launch() enqueues
// the kernels: two steps, so that a caller can make all its requests before it enqueues anything, as hipMalloc beside a busy stream is slow.
struct FuseCells {
    int64_t n = 0, cap = 0;
    unsigned bits = 1;                                          // of a cell key: what a sort by key looks at
    double *part = nullptr, *box = nullptr;
    FuseGrid* grid = nullptr;
    unsigned *keys = nullptr, *idx = nullptr, *skeys = nullptr, *order = nullptr;
    int* cellStart = nullptr;

    int32_t reserve(OneShot& os, size_t& workspace, int64_t rows) {
        auto ws = [&](size_t bytes, auto** p) { workspace += bytes; return os.scratch(bytes, p); };
        n = rows;
        cap = n > 1024 ? n : 1024;
        while (bits < 32 && ((int64_t)1 << bits) < cap) ++bits;
        const size_t un = (size_t)n;
        GSR_TRY(ws((size_t)stride_grid(n) * FUSE_MOM * 8, &part)); GSR_TRY(ws(6 * 8, &box)); GSR_TRY(ws(sizeof(FuseGrid), &grid));
        GSR_TRY(ws(un * 4 + 8, &keys)); GSR_TRY(ws(un * 4 + 8, &idx)); GSR_TRY(ws(un * 4 + 8, &skeys)); GSR_TRY(ws(un * 4 + 8, &order));
        return ws(((size_t)cap + 2) * 4, &cellStart);
    }
    int32_t launch(hipStream_t st, DevBuf& tmp_sort, const float* xyz, const float* cov6, const float* opacity, double* w, double* inv,
                   unsigned long long* n_invalid, double max_distance) {
        const int nblk = stride_grid(n);
        hipLaunchKernelGGL(k_fuse_prep, dim3(stride_grid(n)), dim3(256), 0, st, n, xyz, cov6, opacity, w, inv, n_invalid);
        hipLaunchKernelGGL(k_fuse_moments, dim3(nblk), dim3(256), 0, st, n, xyz, (const double*)w, (const double*)nullptr, part);
        hipLaunchKernelGGL(k_fuse_box, dim3(1), dim3(64), 0, st, nblk, (const double*)part, 0, max_distance, cap, box, grid);
        hipLaunchKernelGGL(k_fuse_moments, dim3(nblk), dim3(256), 0, st, n, xyz, (const double*)w, (const double*)box, part);
        hipLaunchKernelGGL(k_fuse_box, dim3(1), dim3(64), 0, st, nblk, (const double*)part, 1, max_distance, cap, box, grid);
        hipLaunchKernelGGL(k_fuse_keys, dim3(stride_grid(n)), dim3(256), 0, st, n, xyz, (const FuseGrid*)grid, keys, idx);
        if (n > 0) GSR_TRY(sort_pairs_by_key<rocprim::default_config>(tmp_sort, st, (const unsigned*)keys, skeys, (const unsigned*)idx, order, (size_t)n, 0u, bits));
        hipLaunchKernelGGL(k_fuse_cell_starts, dim3(stride_grid(cap + 1)), dim3(256), 0, st, n, (const unsigned*)skeys, cap, cellStart);
        return GSR_OK;
    }
};

}  // namespace gsr
