// gsr_grid.h -- the point grid: the cell-sorted uniform grid over one cloud that every neighbour search of the library walks (the
// HEM, fuse and voxel grids are their own).  GridIndex (host; csrc/grid.hip) builds and owns one; the ICP context holds one for its
// target, the stateless entries (hybrid search, k-NN normals, floater removal) build one over their cloud.  For the kernels: the grid
// record, the cell and slab arithmetic, and the four walks -- expanding rings, a clamped box of row spans, a wave's scan of a span into
// an LDS list, the rank cut of that list -- each written once ("the point grid").  Not part of include/gsr_hip.h.
#pragma once
#include "gsr_common.h"
#include "gsr_features.h"

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
// the cloud has far outliers, GridIndex::build): they are half-infinite slabs.
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

// Expanding rings around (px, py, pz): ring r = the cells at Chebyshev distance r from the point's (clamped) cell, as contiguous
// spans of the sorted points -- a face row of the ring gives its whole x span, an interior row its two end cells.  visit(j, q, d2) for
// every point of every span.  After ring r every unseen point lies beyond a face of that block (faces on the grid boundary have
// nothing behind them), at least `reach` away: stop(reach^2) says whether the caller's list is satisfied by that.  Returns whether
// it stopped (false: rings 0..rmax are walked and it never did).
template <class Visit, class Stop>
__device__ __forceinline__ bool grid_ring_walk(const IcpGrid& g, const int* __restrict__ cellStart, const float4* __restrict__ Tq, double px, double py,
                                               double pz, int rmax, Visit visit, Stop stop) {
    const int cx = icp_cell(px, g.ox, g.inv_c, g.gx), cy = icp_cell(py, g.oy, g.inv_c, g.gy), cz = icp_cell(pz, g.oz, g.inv_c, g.gz);
    // absolute slack of every geometric bound: ~500 ulp of the largest coordinate involved
    const double eps = 1e-13 * (fabs(px) + fabs(py) + fabs(pz) + fabs(g.ox) + fabs(g.oy) + fabs(g.oz) + g.c * (double)(g.gx + g.gy + g.gz));
    for (int r = 0; r <= rmax; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.gz) continue;
            const int adz = dz < 0 ? -dz : dz;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.gy) continue;
                const int ady = dy < 0 ? -dy : dy;
                const int rowbase = (z * g.gy + y) * g.gx;
                const bool face = adz == r || ady == r;
                const int nsp = face ? 1 : 2;
                for (int sidx = 0; sidx < nsp; ++sidx) {
                    int c0, c1;
                    if (face) { c0 = cx - r > 0 ? cx - r : 0; c1 = cx + r < g.gx - 1 ? cx + r : g.gx - 1; }
                    else { c0 = c1 = sidx == 0 ? cx - r : cx + r; }
                    if (c0 < 0 || c1 >= g.gx || c0 > c1) continue;
                    const int s0 = cellStart[rowbase + c0], e0 = cellStart[rowbase + c1 + 1];
                    for (int j = s0; j < e0; ++j) {
                        const float4 q = Tq[j];
                        const double dx = px - (double)q.x, dy2 = py - (double)q.y, dz2 = pz - (double)q.z;
                        visit(j, q, dx * dx + dy2 * dy2 + dz2 * dz2);
                    }
                }
            }
        }
        double reach = 1.0 / 0.0;
        if (cx - r > 0) reach = fmin(reach, px - (g.ox + (double)(cx - r) * g.c));
        if (cx + r < g.gx - 1) reach = fmin(reach, (g.ox + (double)(cx + r + 1) * g.c) - px);
        if (cy - r > 0) reach = fmin(reach, py - (g.oy + (double)(cy - r) * g.c));
        if (cy + r < g.gy - 1) reach = fmin(reach, (g.oy + (double)(cy + r + 1) * g.c) - py);
        if (cz - r > 0) reach = fmin(reach, pz - (g.oz + (double)(cz - r) * g.c));
        if (cz + r < g.gz - 1) reach = fmin(reach, (g.oz + (double)(cz + r + 1) * g.c) - pz);
        reach = reach * 0.999999999 - eps;
        if (reach > 0.0 && stop(reach * reach)) return true;
    }
    return false;
}

// The k best of what is offered, k <= CAP, ascending in (d^2, input index): d^2, sorted position and input index of each.  A thread's
// own list, indexed at run time: it lives in scratch (a list in registers is csrc/clean.hip's k_knn_mean).
#define ICP_KNN 30
template <int CAP>
struct KBest {
    double d[CAP];
    int j[CAP];
    unsigned i[CAP];
    int cnt = 0;
    __device__ __forceinline__ void offer(int k, double d2, int pos_j, unsigned qi) {
        if (cnt == k && !hyb_less(d2, qi, d[cnt - 1], i[cnt - 1])) return;
        int pos = cnt < k ? cnt : k - 1;
        while (pos > 0 && hyb_less(d2, qi, d[pos - 1], i[pos - 1])) {
            d[pos] = d[pos - 1]; j[pos] = j[pos - 1]; i[pos] = i[pos - 1];
            --pos;
        }
        d[pos] = d2; j[pos] = pos_j; i[pos] = qi;
        if (cnt < k) ++cnt;
    }
    // the list holds k entries and the worst of them is strictly closer than every unseen point
    __device__ __forceinline__ bool closed(int k, double reach2) const { return cnt == k && d[cnt - 1] < reach2; }
};

// The rings a box walk needs to hold every point within `radius` of a point of its centre cell
inline int grid_rings_for_radius(const IcpGrid& g, double radius) {
    const double rc = ceil(radius * g.inv_c) + 1.0;                     // +1: a cell index rounded across a boundary
    return rc > (double)(1 << 20) ? (1 << 20) : (int)rc;
}
// The cells within R Chebyshev rings of cell (cx, cy, cz), clamped to the grid: span(s0, e0) = the sorted points of one (y, z) row
template <class Span>
__device__ __forceinline__ void grid_box_walk(const IcpGrid& g, const int* __restrict__ cellStart, int cx, int cy, int cz, int R, Span span) {
    const int z0 = cz - R > 0 ? cz - R : 0, z1 = cz + R < g.gz - 1 ? cz + R : g.gz - 1;
    const int y0 = cy - R > 0 ? cy - R : 0, y1 = cy + R < g.gy - 1 ? cy + R : g.gy - 1;
    const int x0 = cx - R > 0 ? cx - R : 0, x1 = cx + R < g.gx - 1 ? cx + R : g.gx - 1;
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
            const int rowbase = (z * g.gy + y) * g.gx;
            span(cellStart[rowbase + x0], cellStart[rowbase + x1 + 1]);
        }
}

// One wave takes the sorted points [s0, e0) (wave-uniform), 64 at a time, into its LDS list sd / si[0..cnt): the lanes whose point
// passes admit(d2, input index) append by ballot.  When the list would overflow it is cut to the `keep` best by rank, refresh() lets
// the caller tighten what admit() tests against, and the lanes are asked again.
template <class Admit, class Refresh>
__device__ __forceinline__ void wave_scan_take(const float4* __restrict__ Tq, int s0, int e0, double px, double py, double pz, double* sd, unsigned* si,
                                               int& cnt, int keep, Admit admit, Refresh refresh) {
    const int lane = threadIdx.x;
    for (int base = s0; base < e0; base += 64) {
        const int j = base + lane;
        double d2 = 0.0;
        unsigned qi = 0u;
        bool take = false;
        if (j < e0) {
            const float4 q = Tq[j];
            const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
            d2 = dx * dx + dy * dy + dz * dz;
            qi = __float_as_uint(q.w);
            take = admit(d2, qi);
        }
        unsigned long long mask = __ballot(take);
        int nt = __popcll(mask);
        if (cnt + nt > GSR_HYBRID_CAP) {
            cnt = hyb_rank_cut(sd, si, cnt, keep, nullptr);
            refresh();
            take = take && admit(d2, qi);
            mask = __ballot(take);
            nt = __popcll(mask);
        }
        if (take) {
            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            sd[pos] = d2; si[pos] = qi;
        }
        cnt += nt;
        __syncthreads();
    }
}

// ---- host: the index as an object ---------------------------------------------------------------------------------------------
// What a search needs of a built index.  cellStart[ncells + 1]; Tq[n]: the cell-sorted points, the input index in .w (rows with NaN
// coordinates sit in cell 0 and fail every distance comparison) -- a borrower may write to it (csrc/clean.hip takes the rows a stage
// drops out of the search that way).
struct GridView {
    IcpGrid g;
    const int* cellStart;
    float4* Tq;
    int64_t n;
};

// The index over one cloud, and everything it is made with.  The knobs are read from the environment once, here (none changes a
// result): GSR_ICP_CELL_TARGET, GSR_ICP_MAX_CELLS, GSR_ICP_ROBUST_BOX, GSR_ICP_RB_POLL.  Construct it with its device current and
// let it outlive whatever waits for the stream it was built on.
struct GridIndex {
    IcpGrid grid;
    bool robust_box = false;        // the grid lies over the trimmed box (far outliers clamped into the boundary cells)
    DevBuf order, cellStart, Tq;    // order[j] = input index of sorted point j
    GridIndex();
    // bounding box -> robust box -> cell size -> keys, sort, cell starts, gather (+ the normals, when given, into Tn[n]), enqueued on
    // `st`.  Waits for the one or two box read-backs it needs and for nothing else.  max_corr: cells are no finer than max_corr / 64.
    int32_t build(const float* xyz_dev, int64_t n, double max_corr, hipStream_t st, const double* nrm_dev = nullptr, double* Tn = nullptr);
    // order_out[j] = index of the j-th of xyz_dev[n] in the order of THIS grid's cells
    int32_t sort_by_cell(const float* xyz_dev, int64_t n, DevBuf& order_out, hipStream_t st);
    // `bytes` (a multiple of 4, <= 1024) of device memory to the host through the pinned block the host polls; else a copy and a wait
    int32_t fetch(hipStream_t st, const void* dev, void* out, size_t bytes);
    GridView view() const { return {grid, cellStart.as<int>(), Tq.as<float4>(), n}; }
    size_t bytes() const {          // device memory the index holds
        size_t s = 0;
        for (const DevBuf* b : {&bbox, &hist, &keys, &idx, &skeys, &order, &cellStart, &Tq, &rocprim_tmp}) s += b->cap;
        return s;
    }

private:
    int64_t n = 0;
    double cell_target = 2.0;       // target points per grid cell.  Measured at 5M x 5M: 0.5 makes a converged iteration 1.7x faster
                                    // but a cold start (offsets ~ max_corr) 1.6x slower: keep 2
    int max_cells = 1 << 25;
    bool robust_allowed = true;     // GSR_ICP_ROBUST_BOX=0: always the box of all points (test knob: results must not change)
    DevBuf bbox, hist, keys, idx, skeys, rocprim_tmp;
    PinnedBlock host_rb;            // small read-backs: unsigned[256] + the sequence flag; empty = no polling (fetch)
    unsigned long long rb_seq = 0;
};

// gsr_features.h declares hybrid_search_dev (csrc/grid.hip), the stateless search the features, the orientation and the matching use.

}  // namespace gsr
