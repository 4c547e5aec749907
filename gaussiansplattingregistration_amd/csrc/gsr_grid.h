// gsr_grid.h -- the uniform grid of the ICP target index (csrc/icp.hip builds and owns it: gsr_icp_set_target) as seen by the other
// translation units that search it: the grid record, the cell and slab arithmetic every search shares, the LDS rank cut of the
// wave-per-query searches, and how a stateless entry borrows a grid over a cloud of its own (csrc/clean.hip).  Not part of
// include/gsr_hip.h.
#pragma once
#include "gsr_common.h"
#include "gsr_features.h"

struct gsr_icp_ctx;

namespace gsr {

struct IcpGrid {
    double ox, oy, oz, inv_c, c;
    double cx, cy, cz;     // centre used to condition the point-to-point sums
    int gx, gy, gz, ncells;
    int rings;             // ceil(max_corr / c): cells beyond this Chebyshev ring cannot hold an accepted neighbour
    double bx0, by0, bz0, bx1, by1, bz1;      // box of ALL finite target points (the grid may lie over a trimmed one): a query farther from it than max_corr has no neighbour
};

__device__ __forceinline__ int icp_cell(double v, double o, double inv_c, int g) {
    double t = (v - o) * inv_c;
    t = fmin(fmax(t, 0.0), (double)(g - 1));      // NaN -> 0
    return (int)t;
}

// Distance from coordinate v to the slab of cell k along one axis (0 inside), shrunk by a relative 1e-9 so that the
// float64 rounding of the cell classification can never make a bound too large.
// The first and the last cell of an axis also hold every point CLAMPED in from beyond the grid's box (the box is a robust one when
// the cloud has far outliers, gsr_icp_set_target): they are half-infinite slabs.
__device__ __forceinline__ double icp_slab_dist(double v, double o, double c, int k, double eps, int g) {
    const double lo = o + (double)k * c, hi = o + (double)(k + 1) * c;
    const double d = ((v < lo && k > 0) ? lo - v : ((v > hi && k < g - 1) ? v - hi : 0.0)) * 0.999999999 - eps;
    return d > 0.0 ? d : 0.0;
}

__device__ __forceinline__ bool hyb_less(double da, unsigned ia, double db, unsigned ib) { return da < db || (da == db && ia < ib); }

// keeps the min(cnt, keep) best entries of sd / si[0..cnt) at slots 0..keep-1 in (d^2, index) order; returns the new count.
// With `out` the kept entries are written there instead (the final pass).  One wave; the list lives in LDS.
__device__ inline int hyb_rank_cut(double* sd, unsigned* si, int cnt, int keep, int* out) {
    const int lane = threadIdx.x;
    constexpr int PER = GSR_HYBRID_CAP / 64;
    double md[PER];
    unsigned mi[PER];
    int rk[PER];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int e = lane + 64 * t;
        md[t] = e < cnt ? sd[e] : 0.0;
        mi[t] = e < cnt ? si[e] : 0u;
        rk[t] = 0;
    }
    for (int f = 0; f < cnt; ++f) {
        const double fd = sd[f];
        const unsigned fi = si[f];
#pragma unroll
        for (int t = 0; t < PER; ++t) rk[t] += hyb_less(fd, fi, md[t], mi[t]) ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int e = lane + 64 * t;
        if (e < cnt && rk[t] < keep) {
            if (out) out[rk[t]] = (int)mi[t];
            else { sd[rk[t]] = md[t]; si[rk[t]] = mi[t]; }
        }
    }
    __syncthreads();
    return cnt < keep ? cnt : keep;
}

// A grid borrowed by a stateless entry: the index gsr_icp_set_target builds over `xyz_dev` (device memory; rows with NaN
// coordinates sit in cell 0 and fail every distance comparison), enqueued on `stream` and NOT waited for beyond the box read-backs
// the build itself needs.  cellStart[ncells + 1]; Tq[n]: the cell-sorted points, the input index in .w -- the borrower may write to
// it (csrc/clean.hip takes the rows a stage drops out of the search that way).  The context owns everything the view points to:
// gsr_icp_destroy(*ctx) after the stream has been waited for.
struct GridView {
    IcpGrid g;
    const int* cellStart;
    float4* Tq;
    int64_t n;
    size_t bytes;          // device memory the index holds
};
int32_t grid_borrow(const float* xyz_dev, int64_t n, double max_corr, int device, hipStream_t stream, gsr_icp_ctx** ctx, GridView* view);

}  // namespace gsr
