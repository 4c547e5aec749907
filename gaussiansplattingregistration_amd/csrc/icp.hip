// icp.hip -- the per-iteration ICP step on MI355X (gfx950), behind include/gsr_hip.h.
//
// Replaces what the reference reaches through Open3D 0.16.0's registration_icp
// (src/utils/local_registration_util.py:76-100): for every source point, transform, nearest target
// neighbour within max_corr, residual / Jacobian, and the reduction that the estimator solves.
// The reference's Open3D walks a KD-tree per point under OpenMP; here:
//
//   target (once per call)  the point grid of csrc/grid.hip (GridIndex): cell-sorted float4 {x, y, z, bits(input index)},
//                           dense uniform grid (about 2 points per cell, never finer than max_corr/64), prefix table
//                           cellStart[cells+1]; here the optional double3 normals gathered into the same order
//   source (once per call)  sorted by the same grid's cell so that neighbouring lanes walk the same cells
//   k_icp_accumulate<KIND>  ONE fused pass per ICP iteration: p = T*p0 in float64, expanding ring
//                           search over contiguous row spans of the sorted target, exact 1-NN
//                           (ties -> lowest input index), strict d^2 < max_corr^2, residual and
//                           Jacobian, float64 accumulators reduced wave -> block -> per-block
//                           partials; k_fold_partials sums the partials (the fixed order: gsr_fold.h).
//                           No per-point writes; algorithmic bytes 24 (point-to-point) or
//                           48 (point-to-plane, float64 normals) per source point.
//   k_icp_nn                the search alone (thread per point, 56 VGPRs): used with a streaming accumulate kernel
//                           for sources of >= 10^6 points, where occupancy decides (the search is latency bound)
//   estimators              point-to-point (Umeyama), point-to-plane, generalized ICP (W = (Ct + R Cs R^T)^-1/2 per
//                           pair, float64 Jacobi), colored ICP (k_icp_color_gradient prepares the target: 30 nearest
//                           neighbours within 2 max_corr by grid_ring_walk, tangent-plane intensity gradient); robust kernel weights
//   k_icp_accumulate_dev    the same pass for the device-resident loop: T from the device state, the source dealt to the XCDs in
//                           contiguous eighths; eight instantiations (estimator x 27-cell block search)
//   k_icp_step              device-resident loop: reduces the partials, tests convergence, solves (3x3 Jacobi SVD /
//                           6x6 LDL^T) and updates T; the host enqueues chunks of iterations
//   host (this file)        the same solve for the multi-GPU source split (all-reduce callback of 32 doubles).
//
// Accumulator layout (GSR_ICP_ACC_LEN = 32 doubles), see include/gsr_hip.h.
#include "gsr_common.h"
#include "gsr_fold.h"
#include "gsr_normals.h"
#include "gsr_solve.h"
#include "gsr_features.h"
#include "gsr_grid.h"
#include "gsr_oneshot.h"
#include "gsr_test_hooks.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace gsr {
__global__ __launch_bounds__(256) void k_icp_gather_source(int64_t n, const unsigned* __restrict__ order, const float* __restrict__ xyz,
                                                           float* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = order[j];
        out[3 * j] = xyz[3 * i]; out[3 * j + 1] = xyz[3 * i + 1]; out[3 * j + 2] = xyz[3 * i + 2];
    }
}

__global__ __launch_bounds__(256) void k_icp_gather_cov(int64_t n, const unsigned* __restrict__ order, const double* __restrict__ in,
                                                        double* __restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < 6 * n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t / 6;
        const int k = (int)(t - 6 * j);
        out[t] = in[6 * (order ? (int64_t)order[j] : j) + k];
    }
}

struct Xform { double m[12]; };   // rows 0..2 of the 4x4

// Colored ICP operands (KIND 3): target intensity / colour gradient (cell-sorted), source intensity (source order)
struct ColorArgs {
    const double* t_int;
    const double* t_grad;
    const double* s_int;
    double sqrt_lg, sqrt_lp;       // sqrt(lambda_geometric), sqrt(1 - lambda_geometric)
};

// Exact nearest target neighbour of p (float64) by an expanding ring search over the uniform grid.
// Ring r = the cells at Chebyshev distance r from p's (clamped) cell.  Every point in a cell beyond
// ring r is at Euclidean distance >= r*c from p, so the search stops as soon as the best squared
// distance is below (r*c)^2, and never needs to go past ring `rings` = ceil(max_corr / c) because
// farther points cannot be accepted (d^2 < max_corr^2) anyway.  Returns the SORTED position (or -1)
// and d^2; ties go to the lowest input index, as the CPU oracle does.
__device__ __forceinline__ void icp_scan_span(const int* __restrict__ cellStart, const float4* __restrict__ Tq, int first, int last,
                                              double px, double py, double pz, double& bd, int& best, unsigned& best_i) {
    const int s = cellStart[first], e = cellStart[last + 1];
    for (int j = s; j < e; ++j) {
        const float4 q = Tq[j];
        const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
        const double d2 = dx * dx + dy * dy + dz * dz;
        const unsigned qi = __float_as_uint(q.w);
        if (d2 < bd || (d2 == bd && qi < best_i)) { bd = d2; best = j; best_i = qi; }
    }
}

__device__ __forceinline__ void icp_consider(const float4 q, int j, double px, double py, double pz, double& bd, int& best, unsigned& best_i) {
    const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
    const double d2 = dx * dx + dy * dy + dz * dz;
    const unsigned qi = __float_as_uint(q.w);
    if (d2 < bd || (d2 == bd && qi < best_i)) { bd = d2; best = j; best_i = qi; }
}

// BLOCK: rings 0 and 1 as ONE block of 3 x 3 rows of three cells, for the levels whose correspondence distance spans two or
// more cells (the coarse levels of a multiscale run): there the neighbour is rarely in the query's own cell, and the ring
// loop is a chain of dependent loads -- a row's cell bounds, then its points one by one: ~65 round trips to L2 for ~55
// candidates -- with nothing else for the thread to do.  The block loads its 18 cell bounds together and the points four
// at a time (index clamped to the row's last point: a point seen twice changes nothing); any scan order finds the same
// minimum of (d^2, input index), and the ring loop continues at ring 2 when the bound of ring 1 does not close.
// Coarse-to-fine pair of the bench: -11 % at 185 k points, -13 % at 1.67 M.  On a converged fine level (max_corr ~ one
// cell) the neighbour sits in the own cell and the block costs 2.3x: BLOCK = false keeps the ring loop from ring 0.
// Measured and rejected on the coarse levels (185 k - 556 k source points, where the chip is not full): four lanes per query
// (each a z-plane of the block; 1024-thread workgroups), nine rows' loads in flight per lane, and the wave staging the joined
// candidate runs of its 64 neighbouring queries in LDS -- all slower (what they add in registers / LDS costs a
// round of workgroups on the chip, and the kernel's time is its slowest wave, not its average one).
#define ICP_BLOCK_CROWDED 24     // points in a row of the 27-cell block from which on the row is tested against the bound before it is scanned
#ifndef ICP_ROW_BATCH
#define ICP_ROW_BATCH 4
#endif
template <int BLOCK>
__device__ __forceinline__ int icp_nearest(const IcpGrid& g, const int* __restrict__ cellStart,
                                           const float4* __restrict__ Tq, double px, double py, double pz, double& best_d2,
                                           double bound2 = 1.0 / 0.0) {
    // bound2: only a neighbour with d^2 < bound2 is of use to the caller (max_corr^2): the search starts from that bound instead of
    // +inf, so a query with nothing in reach prunes its rings like one that has found something (the outliers of a coarse level
    // walked all (2 rings + 1)^3 cells, one lane holding up its wave)
    int best = -1;
    unsigned best_i = 0xffffffffu;
    double bd = bound2;
    if (!(px == px) || !(py == py) || !(pz == pz)) { best_d2 = 1.0 / 0.0; return -1; }
    {   // a query farther from the box of all target points than the caller's bound has nothing to find: no ring is walked (with a cell of two
        // points and a correspondence distance of many cells -- the reference's default max_correspondence is 5 scene units,
        // registration_parameters.py:9 -- a floater of the source would walk (2 rings + 1)^3 cells and hold up its wave)
        const double ex = fmax(fmax(g.bx0 - px, px - g.bx1), 0.0), ey = fmax(fmax(g.by0 - py, py - g.by1), 0.0), ez = fmax(fmax(g.bz0 - pz, pz - g.bz1), 0.0);
        if ((ex * ex + ey * ey + ez * ez) * 0.999999999 >= bound2) { best_d2 = bound2; return -1; }
    }
    const int cx = icp_cell(px, g.ox, g.inv_c, g.gx), cy = icp_cell(py, g.oy, g.inv_c, g.gy), cz = icp_cell(pz, g.oz, g.inv_c, g.gz);
    // absolute slack of every geometric bound: ~500 ulp of the largest coordinate involved
    const double eps = 1e-13 * (fabs(px) + fabs(py) + fabs(pz) + fabs(g.ox) + fabs(g.oy) + fabs(g.oz) + g.c * (double)(g.gx + g.gy + g.gz));
    int r0 = 0;
    if (BLOCK == 1 && g.rings >= 1) {
        int rs[9], re[9];
        const int xa = cx - 1 > 0 ? cx - 1 : 0, xb = cx + 1 < g.gx - 1 ? cx + 1 : g.gx - 1;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int z = cz + t / 3 - 1, y = cy + t % 3 - 1;
            const bool ok = z >= 0 && z < g.gz && y >= 0 && y < g.gy;
            const int rowbase = ok ? (z * g.gy + y) * g.gx : 0;
            rs[t] = ok ? cellStart[rowbase + xa] : 0;
            re[t] = ok ? cellStart[rowbase + xb + 1] : 0;
        }
        {
        // The query's own row first: its points give the bound a CROWDED neighbour row is tested against before it is scanned.  On
        // a cloud at two points per cell no row is crowded and nothing is tested (the unconditional batched loads are what made the
        // block fast); in a clump -- 45 points per cell on the coarse level of the clustered scene -- a query scanned 1 200 points
        // of which its own row's 135 already held the neighbour.  A row is skipped only when it is STRICTLY farther than the best
        // so far (a point at exactly the best distance could still win the tie on its index).
        constexpr int order9[9] = {4, 1, 3, 5, 7, 0, 2, 6, 8};
#pragma unroll
        for (int tt = 0; tt < 9; ++tt) {
            const int t = order9[tt];
            if (t != 4 && re[t] - rs[t] > ICP_BLOCK_CROWDED) {
                const double dzb = icp_slab_dist(pz, g.oz, g.c, cz + t / 3 - 1, eps, g.gz), dyb = icp_slab_dist(py, g.oy, g.c, cy + t % 3 - 1, eps, g.gy);
                if (dzb * dzb + dyb * dyb > bd) continue;
            }
            // ICP_ROW_BATCH points per round trip; the slots behind the row's end re-read its last point.  (A row of three cells holds
            // ~6 points at two per cell, so four per batch are two dependent round trips per row -- and yet 2, 3 and 4 per batch measure
            // the same, 6 per batch +3 % and 8 per batch +15-35 % on the coarse levels: the registers cost more waves than the shorter
            // chain buys, profiles/archive/r04q_icp_row_batch_ab.txt.)
            for (int j = rs[t]; j < re[t]; j += ICP_ROW_BATCH) {
                const int l = re[t] - 1;
                int jj[ICP_ROW_BATCH];
                float4 qq[ICP_ROW_BATCH];
#pragma unroll
                for (int b = 0; b < ICP_ROW_BATCH; ++b) { jj[b] = j + b < l ? j + b : l; qq[b] = Tq[jj[b]]; }
#pragma unroll
                for (int b = 0; b < ICP_ROW_BATCH; ++b) icp_consider(qq[b], jj[b], px, py, pz, bd, best, best_i);
            }
        }
        }
    }
    if (BLOCK && g.rings >= 1) {
        double reach = 1.0 / 0.0;
        if (cx - 1 > 0) reach = fmin(reach, px - (g.ox + (double)(cx - 1) * g.c));
        if (cx + 1 < g.gx - 1) reach = fmin(reach, (g.ox + (double)(cx + 2) * g.c) - px);
        if (cy - 1 > 0) reach = fmin(reach, py - (g.oy + (double)(cy - 1) * g.c));
        if (cy + 1 < g.gy - 1) reach = fmin(reach, (g.oy + (double)(cy + 2) * g.c) - py);
        if (cz - 1 > 0) reach = fmin(reach, pz - (g.oz + (double)(cz - 1) * g.c));
        if (cz + 1 < g.gz - 1) reach = fmin(reach, (g.oz + (double)(cz + 2) * g.c) - pz);
        reach = reach * 0.999999999 - eps;
        reach = reach > 0.0 ? reach : 0.0;
        if (bd < reach * reach) { best_d2 = bd; return best; }
        r0 = 2;
    }
    for (int r = r0; r <= g.rings; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.gz) continue;
            const int adz = dz < 0 ? -dz : dz;
            const double dzb = icp_slab_dist(pz, g.oz, g.c, z, eps, g.gz);
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.gy) continue;
                const int ady = dy < 0 ? -dy : dy;
                // prune by the best so far: every point of this row is at least (dyb, dzb) away in y / z, and a cell
                // at x-distance dxb adds that.  STRICT comparisons: a candidate at exactly the best distance can still
                // win the tie on its index, so only cells that are strictly farther are skipped.
                const double dyb = icp_slab_dist(py, g.oy, g.c, y, eps, g.gy);
                const double rem = bd - dyb * dyb - dzb * dzb;
                if (rem < 0.0) continue;
                int xlo = 0, xhi = g.gx - 1;
                if (rem < 1e300) {                                // a finite best: clip the x span to |dx| <= sqrt(rem)
                    const double hx = (double)(sqrtf((float)rem) * 1.0001f) + eps + 1e-30;
                    xlo = icp_cell(px - hx, g.ox, g.inv_c, g.gx);
                    xhi = icp_cell(px + hx, g.ox, g.inv_c, g.gx);
                }
                const int rowbase = (z * g.gy + y) * g.gx;
                if (adz == r || ady == r) {                       // a face row of the ring: the whole x span
                    int xa = cx - r > 0 ? cx - r : 0, xb = cx + r < g.gx - 1 ? cx + r : g.gx - 1;
                    xa = xa > xlo ? xa : xlo;
                    xb = xb < xhi ? xb : xhi;
                    if (xa <= xb) icp_scan_span(cellStart, Tq, rowbase + xa, rowbase + xb, px, py, pz, bd, best, best_i);
                } else {                                          // interior row: only the two end cells
                    if (cx - r >= 0 && cx - r >= xlo) icp_scan_span(cellStart, Tq, rowbase + cx - r, rowbase + cx - r, px, py, pz, bd, best, best_i);
                    if (cx + r < g.gx && cx + r <= xhi) icp_scan_span(cellStart, Tq, rowbase + cx + r, rowbase + cx + r, px, py, pz, bd, best, best_i);
                }
            }
        }
        // every cell within Chebyshev distance r has been seen: an unseen point lies beyond one of the faces of that
        // block (faces on the grid boundary have nothing behind them), i.e. at least `reach` away
        double reach = 1.0 / 0.0;
        if (cx - r > 0) reach = fmin(reach, px - (g.ox + (double)(cx - r) * g.c));
        if (cx + r < g.gx - 1) reach = fmin(reach, (g.ox + (double)(cx + r + 1) * g.c) - px);
        if (cy - r > 0) reach = fmin(reach, py - (g.oy + (double)(cy - r) * g.c));
        if (cy + r < g.gy - 1) reach = fmin(reach, (g.oy + (double)(cy + r + 1) * g.c) - py);
        if (cz - r > 0) reach = fmin(reach, pz - (g.oz + (double)(cz - r) * g.c));
        if (cz + r < g.gz - 1) reach = fmin(reach, (g.oz + (double)(cz + r + 1) * g.c) - pz);
        reach = reach * 0.999999999 - eps;
        reach = reach > 0.0 ? reach : 0.0;
        if (bd < reach * reach) break;
    }
    best_d2 = bd;
    return best;
}

// Which source points a workgroup takes.  The source is sorted by the target's cells, so a CONTIGUOUS run of it queries a compact
// region of the target.  Workgroups go to the 8 XCDs round robin: logical block L = (bid % 8) * ceil(nb / 8) + bid / 8 gives every
// XCD one contiguous eighth of the source, and with it an eighth of the target (+ halo) for its own L2 -- block b taking the
// points b * 256 + k * stride made every XCD pull the WHOLE target through its 4 MB (L2 hit rate 46 % on the coarse levels).
// Launch 8 * ceil(nb / 8) workgroups; padding workgroups get nothing.  The partial sums are stored by logical block.
struct IcpRange { int row; int64_t lo, hi; };
__device__ __forceinline__ IcpRange icp_block_range(int64_t ns, int nb, bool remap) {
    int L = (int)blockIdx.x;
    if (remap) {
        const int chunk = (nb + 7) >> 3;
        L = ((int)blockIdx.x & 7) * chunk + ((int)blockIdx.x >> 3);
    }
    const int64_t ppb = ((ns + nb - 1) / nb + 255) / 256 * 256;       // points per logical block, whole waves of a 256-thread block
    IcpRange r;
    r.row = L < nb ? L : -1;
    r.lo = (int64_t)L * ppb;
    r.hi = r.lo + ppb < ns ? r.lo + ppb : ns;
    return r;
}

struct IcpState;
__device__ __forceinline__ bool icp_state_done(const IcpState* st);
__device__ __forceinline__ void icp_state_T(const IcpState* st, double T[12]);

// nn_j[i] = sorted target position of the accepted nearest neighbour of source point i, or -1.  One thread per source
// point: a search kernel with few registers (56 VGPRs, 8 waves per SIMD) in front of a streaming accumulate kernel.
// (Measured and rejected: eight lanes per point with shuffle-combined partial searches -- 1.5x slower.)
template <bool FROM_STATE, int BLOCK>
__global__ __launch_bounds__(256) void k_icp_nn(int64_t ns, const float* __restrict__ src, Xform X, const IcpState* __restrict__ st,
                                                IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq,
                                                double max_corr2, int* __restrict__ nn_j, int nb_logical) {
    double T[12];
    if (FROM_STATE) {
        if (icp_state_done(st)) return;
        icp_state_T(st, T);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = X.m[i];
    }
    const IcpRange rg = icp_block_range(ns, nb_logical < 0 ? -nb_logical : nb_logical, nb_logical > 0);
    if (rg.row < 0) return;
    for (int64_t i = rg.lo + threadIdx.x; i < rg.hi; i += blockDim.x) {
        const double x = (double)src[3 * i], y = (double)src[3 * i + 1], z = (double)src[3 * i + 2];
        const double px = T[0] * x + T[1] * y + T[2] * z + T[3];
        const double py = T[4] * x + T[5] * y + T[6] * z + T[7];
        const double pz = T[8] * x + T[9] * y + T[10] * z + T[11];
        double d2;
        const int j = icp_nearest<BLOCK>(g, cellStart, Tq, px, py, pz, d2, max_corr2);
        nn_j[i] = (j >= 0 && d2 < max_corr2) ? j : -1;
    }
}

__device__ __forceinline__ double icp_weight(int loss, double k, double r) {   // Open3D RobustKernel.cpp
    switch (loss) {
        case GSR_LOSS_TUKEY: { double t = fmin(1.0, fabs(r) / k); double u = 1.0 - t * t; return u * u; }
        case GSR_LOSS_CAUCHY: { double t = r / k; return 1.0 / (1.0 + t * t); }
        case GSR_LOSS_GM: { double t = k + r * r; return k / (t * t); }
        case GSR_LOSS_HUBER: { double e = fabs(r); return k / fmax(e, k); }
        default: return 1.0;
    }
}

// Symmetric 3x3 eigen-decomposition (cyclic Jacobi, float64): A = V diag(lam) V^T.
__host__ __device__ static void sym_eig3(double a00, double a01, double a02, double a11, double a12, double a22, double V[3][3], double lam[3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dg = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-40 * dg)) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - sn * y; A[k][q] = sn * x + c * y; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - sn * y; A[q][k] = sn * x + c * y; }
#pragma unroll
                for (int k = 0; k < 3; ++k) { const double x = V[k][p], y = V[k][q]; V[k][p] = c * x - sn * y; V[k][q] = sn * x + c * y; }
            }
    }
    lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
}

// Generalized ICP (Open3D GeneralizedICP.cpp, ComputeTransformation): three residual rows of one matched pair into
// acc[2..29].  cs6 = the source covariance in the ORIGINAL frame (rotated here by R = T[0:3,0:3]), ct6 = target's.
template <int NACC>
__device__ __forceinline__ void icp_gicp_rows(double (&acc)[NACC], const double* T, double px, double py, double pz, double qx, double qy,
                                              double qz, const double* __restrict__ cs6, const double* __restrict__ ct6, int loss, double kparam) {
    const double c0[3][3] = {{cs6[0], cs6[1], cs6[2]}, {cs6[1], cs6[3], cs6[4]}, {cs6[2], cs6[4], cs6[5]}};
    const double R[3][3] = {{T[0], T[1], T[2]}, {T[4], T[5], T[6]}, {T[8], T[9], T[10]}};
    double RC[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) RC[a][b] = R[a][0] * c0[0][b] + R[a][1] * c0[1][b] + R[a][2] * c0[2][b];
    double M[6];                                   // Ct + R Cs R^T, upper triangle
    {
        int t = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b) { M[t] = ct6[t] + (RC[a][0] * R[b][0] + RC[a][1] * R[b][1] + RC[a][2] * R[b][2]); ++t; }
    }
    double V[3][3], lam[3], W[3][3];
    sym_eig3(M[0], M[1], M[2], M[3], M[4], M[5], V, lam);
    const double is[3] = {1.0 / sqrt(lam[0]), 1.0 / sqrt(lam[1]), 1.0 / sqrt(lam[2])};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) W[a][b] = V[a][0] * is[0] * V[b][0] + V[a][1] * is[1] * V[b][1] + V[a][2] * is[2] * V[b][2];
    const double d[3] = {px - qx, py - qy, pz - qz};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        // J_i = [ (W * -skew(p)).row(i), W.row(i) ],  -skew(p) = [[0, pz, -py], [-pz, 0, px], [py, -px, 0]]
        const double J[6] = {W[i][1] * -pz + W[i][2] * py, W[i][0] * pz + W[i][2] * -px, W[i][0] * -py + W[i][1] * px,
                             W[i][0], W[i][1], W[i][2]};
        const double r = W[i][0] * d[0] + W[i][1] * d[1] + W[i][2] * d[2];
        const double w = icp_weight(loss, kparam, r);
        int t = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[t++] += J[a] * w * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[23 + a] += J[a] * w * r;
        acc[29] += r * r;
    }
}

// Colored ICP (Open3D ColoredICP.cpp, ComputeTransformation): the geometric and the photometric row of one pair.
template <int NACC>
__device__ __forceinline__ void icp_colored_rows(double (&acc)[NACC], const ColorArgs& ca, double px, double py, double pz, double qx, double qy,
                                                 double qz, double nx, double ny, double nz, int64_t i, int64_t j, int loss, double kparam) {
    const double dn = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;
    double J[2][6], r[2];
    J[0][0] = ca.sqrt_lg * (py * nz - pz * ny); J[0][1] = ca.sqrt_lg * (pz * nx - px * nz); J[0][2] = ca.sqrt_lg * (px * ny - py * nx);
    J[0][3] = ca.sqrt_lg * nx; J[0][4] = ca.sqrt_lg * ny; J[0][5] = ca.sqrt_lg * nz;
    r[0] = ca.sqrt_lg * dn;
    const double pjx = px - dn * nx - qx, pjy = py - dn * ny - qy, pjz = pz - dn * nz - qz;      // vs_proj - vt
    const double d0 = ca.t_grad[3 * j], d1 = ca.t_grad[3 * j + 1], d2 = ca.t_grad[3 * j + 2];
    const double is0 = d0 * pjx + d1 * pjy + d2 * pjz + ca.t_int[j];
    const double dd = d0 * nx + d1 * ny + d2 * nz;
    const double m0 = -(d0 - dd * nx), m1 = -(d1 - dd * ny), m2 = -(d2 - dd * nz);               // -dit^T (I - n n^T)
    J[1][0] = ca.sqrt_lp * (py * m2 - pz * m1); J[1][1] = ca.sqrt_lp * (pz * m0 - px * m2); J[1][2] = ca.sqrt_lp * (px * m1 - py * m0);
    J[1][3] = ca.sqrt_lp * m0; J[1][4] = ca.sqrt_lp * m1; J[1][5] = ca.sqrt_lp * m2;
    r[1] = ca.sqrt_lp * (ca.s_int[i] - is0);
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const double w = icp_weight(loss, kparam, r[row]);
        int t = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[t++] += J[row][a] * w * J[row][b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[23 + a] += J[row][a] * w * r[row];
        acc[29] += r[row] * r[row];
    }
}

// Colour gradient of every target point (Open3D InitializePointCloudForColoredICP): its ICP_KNN nearest neighbours
// (itself first) within `radius`, ordered by (distance, input index); with >= 4 of them a 3x3 least-squares fit of the
// intensity differences over the tangent-plane projections, plus the orthogonality row (nn-1) n.  One thread per
// point: grid_ring_walk into a KBest list (gsr_grid.h).
__global__ __launch_bounds__(256) void k_icp_color_gradient(int64_t nt, IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq,
                                                            const double* __restrict__ Tn, const double* __restrict__ t_int, double radius,
                                                            double* __restrict__ t_grad) {
    for (int64_t jq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; jq < nt; jq += (int64_t)gridDim.x * blockDim.x) {
        const float4 qv = Tq[jq];
        const double px = (double)qv.x, py = (double)qv.y, pz = (double)qv.z;
        t_grad[3 * jq] = 0.0; t_grad[3 * jq + 1] = 0.0; t_grad[3 * jq + 2] = 0.0;
        if (!(px == px) || !(py == py) || !(pz == pz)) continue;
        KBest<ICP_KNN> kb;
        const double r2 = radius * radius;
        // done when the list is full and its worst entry is strictly closer than every unseen point, or when the radius is covered
        grid_ring_walk(g, cellStart, Tq, px, py, pz, (int)ceil(radius / g.c) + 1,
                       [&](int j, const float4& q, double d2) { if (d2 < r2) kb.offer(ICP_KNN, d2, j, __float_as_uint(q.w)); },      // the hybrid search keeps d^2 < radius^2
                       [&](double reach2) { return kb.closed(ICP_KNN, reach2) || r2 < reach2; });
        const int cnt = kb.cnt;
        const int* kj = kb.j;
        if (cnt < 4) continue;
        const double nx = Tn[3 * jq], ny = Tn[3 * jq + 1], nz = Tn[3 * jq + 2];
        const double it = t_int[jq];
        double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, b[3] = {0, 0, 0};
        for (int i = 1; i < cnt; ++i) {
            const float4 q = Tq[kj[i]];
            const double vx = (double)q.x - px, vy = (double)q.y - py, vz = (double)q.z - pz;
            const double dn = vx * nx + vy * ny + vz * nz;
            const double row[3] = {(double)q.x - dn * nx - px, (double)q.y - dn * ny - py, (double)q.z - dn * nz - pz};
            const double rhs = t_int[kj[i]] - it;
            for (int p = 0; p < 3; ++p) { for (int c2 = 0; c2 < 3; ++c2) A[p][c2] += row[p] * row[c2]; b[p] += row[p] * rhs; }
        }
        const double f = (double)(cnt - 1);
        const double row[3] = {f * nx, f * ny, f * nz};
        for (int p = 0; p < 3; ++p) for (int c2 = 0; c2 < 3; ++c2) A[p][c2] += row[p] * row[c2];
        // 3x3 solve: Gaussian elimination with partial pivoting
        double M[3][4] = {{A[0][0], A[0][1], A[0][2], b[0]}, {A[1][0], A[1][1], A[1][2], b[1]}, {A[2][0], A[2][1], A[2][2], b[2]}};
        for (int c2 = 0; c2 < 3; ++c2) {
            int piv = c2;
            for (int rr = c2 + 1; rr < 3; ++rr) if (fabs(M[rr][c2]) > fabs(M[piv][c2])) piv = rr;
            for (int k2 = 0; k2 < 4; ++k2) { const double tmp = M[c2][k2]; M[c2][k2] = M[piv][k2]; M[piv][k2] = tmp; }
            for (int rr = c2 + 1; rr < 3; ++rr) {
                const double fct = M[rr][c2] / M[c2][c2];
                for (int k2 = c2; k2 < 4; ++k2) M[rr][k2] -= fct * M[c2][k2];
            }
        }
        double x[3];
        for (int i = 2; i >= 0; --i) {
            double v = M[i][3];
            for (int k2 = i + 1; k2 < 3; ++k2) v -= M[i][k2] * x[k2];
            x[i] = v / M[i][i];
        }
        t_grad[3 * jq] = x[0]; t_grad[3 * jq + 1] = x[1]; t_grad[3 * jq + 2] = x[2];
    }
}
// intensity = mean of the three colour channels (float64), gathered into `order` (NULL = identity)
__global__ __launch_bounds__(256) void k_icp_intensity(int64_t n, const unsigned* __restrict__ order, const double* __restrict__ rgb,
                                                       double* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = order ? (int64_t)order[j] : j;
        out[j] = (rgb[3 * i] + rgb[3 * i + 1] + rgb[3 * i + 2]) / 3.0;
    }
}

// KIND 0: point-to-point sums (17 values); KIND 1: point-to-plane normal equations (30 values); KIND 4: kind 0's 17 sums in the same
// order plus slot 17 = sum |a|^2 (18 values) -- an instantiation of its own: the kind-0 kernels carry no trace of it
constexpr int icp_nacc(int kind) { return kind == 0 ? 17 : (kind == 4 ? 18 : 30); }

// One accepted correspondence: source row i moved to p = T p0, matched to the target's sorted row j.  Both accumulate kernels call
// this; they differ only in where T lives (a kernel argument, the device-resident state).
template <int KIND>
__device__ __forceinline__ void icp_rows(double (&acc)[icp_nacc(KIND)], const double* T, const IcpGrid& g, const float4* __restrict__ Tq,
                                         const double* __restrict__ Tn, const double* __restrict__ Sc, const ColorArgs& ca, double px, double py,
                                         double pz, int64_t i, int j, int loss, double kparam) {
    constexpr int NACC = icp_nacc(KIND);
    const float4 q = Tq[j];
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const double ddx = px - qx, ddy = py - qy, ddz = pz - qz;
    const double d2 = ddx * ddx + ddy * ddy + ddz * ddz;
    acc[0] += 1.0;
    acc[1] += d2;
    if constexpr (KIND == 0 || KIND == 4) {
        const double ax = px - g.cx, ay = py - g.cy, az = pz - g.cz;
        const double bx = qx - g.cx, by = qy - g.cy, bz = qz - g.cz;
        acc[2] += ax; acc[3] += ay; acc[4] += az;
        acc[5] += bx; acc[6] += by; acc[7] += bz;
        acc[8] += ax * bx; acc[9] += ax * by; acc[10] += ax * bz;
        acc[11] += ay * bx; acc[12] += ay * by; acc[13] += ay * bz;
        acc[14] += az * bx; acc[15] += az * by; acc[16] += az * bz;
        if constexpr (KIND == 4) acc[17] += ax * ax + ay * ay + az * az;        // Umeyama's source variance (with_scaling)
    } else if constexpr (KIND == 2) {
        icp_gicp_rows<NACC>(acc, T, px, py, pz, qx, qy, qz, Sc + 6 * i, Tn + 6 * (int64_t)j, loss, kparam);
    } else if constexpr (KIND == 3) {
        icp_colored_rows<NACC>(acc, ca, px, py, pz, qx, qy, qz, Tn[3 * (int64_t)j], Tn[3 * (int64_t)j + 1], Tn[3 * (int64_t)j + 2], i, j, loss, kparam);
    } else {
        const double nx = Tn[3 * (int64_t)j], ny = Tn[3 * (int64_t)j + 1], nz = Tn[3 * (int64_t)j + 2];
        const double r = (px - qx) * nx + (py - qy) * ny + (pz - qz) * nz;
        const double w = icp_weight(loss, kparam, r);
        const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
        int t = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[t++] += J[a] * w * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[23 + a] += J[a] * w * r;
        acc[29] += r * r;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_icp_accumulate(int64_t ns, const float* __restrict__ src, Xform T, IcpGrid g,
                                                        const int* __restrict__ cellStart, const int* __restrict__ nn_j,
                                                        const float4* __restrict__ Tq, const double* __restrict__ Tn,
                                                        const double* __restrict__ Sc, ColorArgs ca, double max_corr2,
                                                        int loss, double kparam, double* __restrict__ partials) {
    constexpr int NACC = icp_nacc(KIND);
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = (double)src[3 * i], y = (double)src[3 * i + 1], z = (double)src[3 * i + 2];
        const double px = T.m[0] * x + T.m[1] * y + T.m[2] * z + T.m[3];
        const double py = T.m[4] * x + T.m[5] * y + T.m[6] * z + T.m[7];
        const double pz = T.m[8] * x + T.m[9] * y + T.m[10] * z + T.m[11];
        int j;
        if (nn_j) {                                 // optional two-kernel form: neighbours from k_icp_nn (accepted or -1)
            j = nn_j[i];
            if (j < 0) continue;
        } else {
            double dd;
            j = icp_nearest<0>(g, cellStart, Tq, px, py, pz, dd, max_corr2);
            if (j < 0 || !(dd < max_corr2)) continue;
        }
        icp_rows<KIND>(acc, T.m, g, Tq, Tn, Sc, ca, px, py, pz, i, j, loss, kparam);
    }
    block_fold_store<NACC, GSR_ICP_ACC_LEN, wave_sum_rows>(acc, partials, (int)blockIdx.x);
}

// Information matrix of a registered pair (gsr_icp_information): Lambda = sum G^T G over the correspondences, G = [-[q]x | I3] at the
// matched TARGET point q, depends on them only through n, sum q and sum q q^T -- ten float64 sums per lane (the 6x6 is put together on
// the host).  A kernel of its own, not a KIND of k_icp_accumulate: that template's instantiations keep their registers.  Same search as
// an evaluation (fused icp_nearest, or nn_j from k_icp_nn), same grid, same fold: bit-reproducible, no atomics.
#define ICP_INFO_NACC 10
__global__ __launch_bounds__(256) void k_icp_information(int64_t ns, const float* __restrict__ src, Xform T, IcpGrid g,
                                                         const int* __restrict__ cellStart, const int* __restrict__ nn_j,
                                                         const float4* __restrict__ Tq, double max_corr2, double* __restrict__ partials) {
    double acc[ICP_INFO_NACC];
#pragma unroll
    for (int k = 0; k < ICP_INFO_NACC; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (int64_t)gridDim.x * blockDim.x) {
        int j;
        if (nn_j) {
            j = nn_j[i];
            if (j < 0) continue;
        } else {
            const double x = (double)src[3 * i], y = (double)src[3 * i + 1], z = (double)src[3 * i + 2];
            const double px = T.m[0] * x + T.m[1] * y + T.m[2] * z + T.m[3];
            const double py = T.m[4] * x + T.m[5] * y + T.m[6] * z + T.m[7];
            const double pz = T.m[8] * x + T.m[9] * y + T.m[10] * z + T.m[11];
            double dd;
            j = icp_nearest<0>(g, cellStart, Tq, px, py, pz, dd, max_corr2);
            if (j < 0 || !(dd < max_corr2)) continue;
        }
        const float4 q = Tq[j];
        const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
        acc[0] += 1.0;
        acc[1] += qx; acc[2] += qy; acc[3] += qz;
        acc[4] += qx * qx; acc[5] += qx * qy; acc[6] += qx * qz;
        acc[7] += qy * qy; acc[8] += qy * qz; acc[9] += qz * qz;
    }
    block_fold_store<ICP_INFO_NACC, GSR_ICP_ACC_LEN, wave_sum_rows>(acc, partials, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void k_icp_correspond(int64_t ns, const float* __restrict__ src, Xform T, const int* __restrict__ nn_j,
                                                        const float4* __restrict__ Tq, const unsigned* __restrict__ src_order,
                                                        int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ns; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = src_order ? (int64_t)src_order[k] : k;          // results go back to the caller's order
        const int j = nn_j[k];
        if (j < 0) { out_idx[i] = -1; out_d2[i] = 0.0; continue; }
        const double x = (double)src[3 * k], y = (double)src[3 * k + 1], z = (double)src[3 * k + 2];
        const double px = T.m[0] * x + T.m[1] * y + T.m[2] * z + T.m[3];
        const double py = T.m[4] * x + T.m[5] * y + T.m[6] * z + T.m[7];
        const double pz = T.m[8] * x + T.m[9] * y + T.m[10] * z + T.m[11];
        const float4 q = Tq[j];
        const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
        out_idx[i] = (int64_t)__float_as_uint(q.w);
        out_d2[i] = dx * dx + dy * dy + dz * dz;
    }
}

// ---- normals from splat covariances: gsr_normals.h (shared with hem.hip: the normals of a level leave with the level)
__global__ __launch_bounds__(256) void k_normals_from_cov(int64_t n, const float* __restrict__ cov6, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v[3];
        normal_of_cov_d(cov6[6 * i], cov6[6 * i + 1], cov6[6 * i + 2], cov6[6 * i + 3], cov6[6 * i + 4], cov6[6 * i + 5], v);
        out[3 * i] = v[0]; out[3 * i + 1] = v[1]; out[3 * i + 2] = v[2];
    }
}

// Covariances of a cloud that has none, for generalized ICP (Open3D GeneralizedICP.cpp, InitializePointCloudForGeneralizedICP):
// C_i = Rx diag(epsilon, 1, 1) Rx^T with Rx = GetRotationFromE1ToX(n_i) = I + [v]x + [v]x^2 / (1 + c), v = e1 x n_i, c = e1 . n_i
// (the identity when c < -0.99, as Open3D has it).  The reference reaches this with its SPARSE input clouds, which carry KNN-30
// normals but no covariances (point_cloud_converter.py:9-28, qt_multiscale_registrator.py:82-85).  cov6 out: xx xy xz yy yz zz.
__global__ __launch_bounds__(256) void k_cov_from_normals(int64_t n, const double* __restrict__ nrm, double eps, double* __restrict__ cov6) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = nrm[3 * i], y = nrm[3 * i + 1], z = nrm[3 * i + 2];
        double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        const double c = x;                                   // e1 . n
        if (!(c < -0.99)) {
            const double v[3] = {0.0, -z, y};                 // e1 x n
            const double sv[3][3] = {{0, -v[2], v[1]}, {v[2], 0, -v[0]}, {-v[1], v[0], 0}};
            const double f = 1.0 / (1.0 + c);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    double sq = 0;
                    for (int k = 0; k < 3; ++k) sq += sv[a][k] * sv[k][b];
                    R[a][b] = (a == b ? 1.0 : 0.0) + sv[a][b] + sq * f;
                }
        }
        const double d[3] = {eps, 1.0, 1.0};
        int t = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                // (Rx * C) * Rx^T in Eigen's evaluation order: the product with the diagonal first
                double sum = 0;
                for (int k = 0; k < 3; ++k) sum += (R[a][k] * d[k]) * R[b][k];
                cov6[6 * i + t++] = sum;
            }
    }
}


// ---- device-resident ICP loop -------------------------------------------------------------------------
// registration_icp's loop needs, per iteration, one correspondence pass and a 3x3 / 6x6 solve on 32
// doubles.  Driving it from the host costs a device->host copy and a stream synchronisation per
// iteration (~60 us, comparable to the kernel itself on small levels); here the transform, the
// convergence test and the solve stay on the device: k_icp_accumulate_dev reads T from IcpState,
// k_icp_step reduces the block partials (the fixed order of gsr_fold.h), tests convergence,
// solves and updates T in ONE thread.  The host enqueues iterations in chunks and looks at `done` once
// per chunk; iterations enqueued after convergence return immediately.
struct IcpState {
    double T[16];
    double fit, rmse;          // of the latest evaluation
    double ctr[3], nsg, rel_fit, rel_rmse;
    int iters, done, max_iter, kind, evals;
};

__device__ __forceinline__ bool icp_state_done(const IcpState* st) { return st->done != 0; }
__device__ __forceinline__ void icp_state_T(const IcpState* st, double T[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = st->T[i];
}

// One evaluation of the device-resident loop: the block partials of this iteration's sums, by logical block.  k_icp_step (single
// GPU) or k_icp_reduce + the all-reduce + k_icp_step (multi-GPU source split) follow as their own launches.
template <int KIND, int BLOCK>
__global__ __launch_bounds__(256, 1) void k_icp_accumulate_dev(int64_t ns, const float* __restrict__ src, IcpState* st,
                                                            IcpGrid g, const int* __restrict__ cellStart, const int* __restrict__ nn_j,
                                                            const float4* __restrict__ Tq, const double* __restrict__ Tn,
                                                            const double* __restrict__ Sc, ColorArgs ca, double max_corr2,
                                                            int loss, double kparam, double* partials, int nb_logical) {
    constexpr int NACC = icp_nacc(KIND);
    const IcpRange rg = icp_block_range(ns, nb_logical < 0 ? -nb_logical : nb_logical, nb_logical > 0);
    if (st->done) return;                           // converged: nothing to search
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = st->T[i];
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    if (rg.row < 0) return;                         // (a padding workgroup of the XCD mapping)
    for (int64_t i = rg.lo + threadIdx.x; i < rg.hi; i += blockDim.x) {
        const double x = (double)src[3 * i], y = (double)src[3 * i + 1], z = (double)src[3 * i + 2];
        const double px = T[0] * x + T[1] * y + T[2] * z + T[3];
        const double py = T[4] * x + T[5] * y + T[6] * z + T[7];
        const double pz = T[8] * x + T[9] * y + T[10] * z + T[11];
        int j;
        if (nn_j) {                                 // optional two-kernel form: neighbours from k_icp_nn (accepted or -1)
            j = nn_j[i];
            if (j < 0) continue;
        } else {
            double dd;
            j = icp_nearest<BLOCK>(g, cellStart, Tq, px, py, pz, dd, max_corr2);
            if (j < 0 || !(dd < max_corr2)) continue;
        }
        icp_rows<KIND>(acc, T, g, Tq, Tn, Sc, ca, px, py, pz, i, j, loss, kparam);
    }
    block_fold_store<NACC, GSR_ICP_ACC_LEN, wave_sum_rows>(acc, partials, rg.row);
}

// `reduced` == NULL: fold the block partials here (single GPU).  Multi-GPU source split: k_icp_reduce folds them into a
// device vector, the all-reduce callback sums that vector over the ranks (RCCL, on this stream), and this kernel starts
// from the reduced vector -- every rank then takes the identical decision and the identical update.
// 512 threads: the single-thread solve behind the reduction needs ~150 registers (a 1024-thread launch bound allows 128: it
// spilled to scratch).
#define ICP_STEP_THREADS 512
// k_fold_partials<64>'s sums, bit for bit (the order: gsr_fold.h), read as rows: with THREADS = 32 G threads, thread (g = t / 32,
// k = t % 32) forms the lane sums s_g, s_(g + G), ... of accumulator k (32 threads read one 256-byte row per load, four rounds of
// loads in flight; a wave per accumulator read 8 bytes of 64 different rows), folds the steps of the tree it holds both operands of,
// and an LDS tree over g does the remaining log2 G.  Result: s_x[0][k].
template <int THREADS>
__device__ __forceinline__ void icp_fold_partials(int nblocks, const double* partials, const double* __restrict__ reduced, double (*s_x)[32]) {
    constexpr int G = THREADS / 32, NL = 64 / G;
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (reduced) {
        if (g == 0) s_x[0][k] = reduced[k];
        __syncthreads();
        return;
    }
    double sl[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) sl[j] = 0.0;
    for (int b0 = g; b0 < nblocks; b0 += 256) {
        double v[4][NL];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int b = b0 + 64 * u + G * j;
                v[u][j] = b < nblocks ? partials[(int64_t)b * GSR_ICP_ACC_LEN + k] : 0.0;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (b0 + 64 * u + G * j < nblocks) sl[j] += v[u][j];
    }
#pragma unroll
    for (int h = NL / 2; h >= 1; h >>= 1)                   // butterfly steps 32, 16, ... between the lanes this thread holds
#pragma unroll
        for (int j = 0; j < h; ++j) sl[j] = sl[j] + sl[j + h];
    s_x[g][k] = sl[0];
    __syncthreads();
    for (int o = G / 2; o > 0; o >>= 1) {
        if (g < o) s_x[g][k] = s_x[g][k] + s_x[g + o][k];
        __syncthreads();
    }
}
// one thread: fitness / RMSE, the relative-change test, the estimator's solve and T <- update * T (registration_icp's loop body)
__device__ __forceinline__ void icp_step_solve(const double* acc32, const IcpState& s_st, IcpState* st) {
    double acc[GSR_ICP_ACC_LEN];
#pragma unroll
    for (int i = 0; i < GSR_ICP_ACC_LEN; ++i) acc[i] = acc32[i];
    const double fit = acc[0] > 0 ? acc[0] / s_st.nsg : 0.0, rmse = acc[0] > 0 ? sqrt(acc[1] / acc[0]) : 0.0;
    const bool first = s_st.evals == 0;
    const bool stop = !first && fabs(s_st.fit - fit) < s_st.rel_fit && fabs(s_st.rmse - rmse) < s_st.rel_rmse;
    st->fit = fit; st->rmse = rmse;
    st->evals = s_st.evals + 1;
    if (stop || s_st.iters >= s_st.max_iter) { st->done = 1; return; }
    double update[16], T[16];
    estimate_update(s_st.ctr, s_st.kind, acc, update);
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = s_st.T[i];
    mat4_mul(update, T, T);
#pragma unroll
    for (int i = 0; i < 16; ++i) st->T[i] = T[i];
    st->iters = s_st.iters + 1;
}
// 512 threads: the single-thread solve behind the reduction needs ~120 registers (a 1024-thread launch bound allows 128: it
// spilled to scratch)
__global__ __launch_bounds__(ICP_STEP_THREADS) void k_icp_step(int nblocks, const double* __restrict__ partials, const double* __restrict__ reduced,
                                                   IcpState* __restrict__ st) {
    __shared__ double s_x[16][GSR_ICP_ACC_LEN];
    __shared__ IcpState s_st;
    static_assert(GSR_ICP_ACC_LEN == 32 && sizeof(IcpState) % 4 == 0, "k_icp_step layout");
    if (threadIdx.x < sizeof(IcpState) / 4) reinterpret_cast<int*>(&s_st)[threadIdx.x] = reinterpret_cast<const int*>(st)[threadIdx.x];
    icp_fold_partials<ICP_STEP_THREADS>(nblocks, partials, reduced, s_x);
    if (threadIdx.x != 0 || s_st.done) return;
    icp_step_solve(&s_x[0][0], s_st, st);
}

// rank-local accumulator vector of one iteration (k_fold_partials<64>'s sums, 16 waves over the 32 of them); zeros once converged, so
// that the ranks keep calling the collective in step
__global__ __launch_bounds__(1024) void k_icp_reduce(int nblocks, const double* __restrict__ partials, const IcpState* __restrict__ st,
                                                     double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool done = st->done != 0;
    for (int k = wv; k < GSR_ICP_ACC_LEN; k += 16) {
        double s = 0.0;
        if (!done)
            for (int b = lane; b < nblocks; b += 64) s += partials[(int64_t)b * GSR_ICP_ACC_LEN + k];
        s = wave_sum_xor(s);
        if (lane == 0) out[k] = s;
    }
}

// gsr_debug_fold: thread t of block b holds row 256 b + t of x [n][3], zeros past n; block_fold_store and nothing else
template <double (*WaveSum)(double)>
__global__ __launch_bounds__(256) void k_debug_fold(int64_t n, const double* __restrict__ x, double* __restrict__ partials) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double acc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = i < n ? x[3 * i + k] : 0.0;
    block_fold_store<3, 4, WaveSum>(acc, partials, (int)blockIdx.x);
}

}  // namespace gsr

using namespace gsr;

struct gsr_icp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    GridIndex index;                // the target's point grid: cells, cellStart, the sorted points Tq, order (gsr_grid.h)
    bool have_target = false, have_normals = false, have_source = false;
    int64_t nt = 0, ns = 0, ns_global = 0;
    double max_corr = 0;
    DevBuf src_raw, src_order, state, nn_j, Tc, Sc, stage_cov, Ti, Tg, Si;
    bool have_tcov = false, have_scov = false, have_tcol = false, have_scol = false;
    double lambda_geometric = 0.968;            // Open3D TransformationEstimationForColoredICP default
    bool src_sorted = false;
    bool device_loop = true;        // GSR_ICP_DEVICE_LOOP=0 selects the host-driven loop
    bool block_search = true;       // GSR_ICP_BLOCK_SEARCH=0: always the ring loop from ring 0
    bool xcd_ranges = true;         // GSR_ICP_XCD=0: logical block = physical block (every XCD walks the whole source)
    gsr_comm* comm = nullptr;       // multi-GPU source split through a communicator (gsr_icp_set_comm)
    // Search / accumulate split (GSR_ICP_NN_KERNEL): 0 = one fused kernel (120 VGPRs with the 30 float64 accumulators:
    // 4 waves per SIMD); 2 = a thread-per-point search kernel (56 VGPRs, 8 waves per SIMD) writes nn_j and a streaming
    // kernel accumulates -- the search is latency bound, so occupancy wins: 21 % faster at 5 M points, equal at 0.5 M,
    // 8 % slower at 0.2 M (one more launch).  -1 = choose by size (the default).  Same results either way
    // (tests/test_icp_gpu.py::test_icp_knobs_change_nothing).
    int nn_kernel = -1;
    // the search in its own kernel (k_icp_nn, few registers, full occupancy) + a streaming accumulate from 400 k source points on:
    // measured on the bench's levels with the XCD-contiguous ranges, fused / split: 185 k 51.7 / 59.2 us, 556 k 90.1 / 81.6, 1.67 M 233 / 190,
    // 5 M 563 / 397 per iteration
    int nn_mode() const { return nn_kernel >= 0 ? (nn_kernel ? 2 : 0) : (ns >= 400000 ? 2 : 0); }
    DevBuf Tn, stage_xyz, stage_nrm, src, partials, acc_dev, corr_idx, corr_d2;
    gsr_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    gsr_allreduce_dev64_fn allreduce_dev = nullptr;      // device-resident loop with a stream-ordered collective per iteration
    void* allreduce_dev_user = nullptr;
    Event e0, e1, eb0, eb1;         // e0 / e1: the iteration loop; eb0 / eb1: the target index build
    bool defer_sync = false;        // gsr_icp_register_clouds: set_target / set_source do not wait for the stream (the registration behind them does)
    bool build_pending = false;     // ms_build has not been read from eb0 / eb1 yet
    float ms_build = 0, ms_iter = 0;
    int n_iter_kernels = 0;
    // workgroups of the search + accumulate kernel: three fit a CU (141 VGPRs), 768 are ONE round on the chip.  With 1 024 the last
    // 256 ran as a second, quarter-full round: 108 -> 95 us per iteration at 556 k source points (GSR_ICP_BLOCKS)
    int nblocks = 768;
    ~gsr_icp_ctx() { (void)hipSetDevice(device); }     // the members free themselves, on the context's device
};

namespace {

// Logical blocks for ns points when at most `cap` workgroups are wanted: every block takes a whole number of 256-point trips
// (icp_block_range), and there are exactly as many blocks as have points -- the XCD mapping deals them out in eighths, so
// blocks without work at the end would leave whole XCDs idle.
inline int icp_blocks(int64_t ns, int cap) {
    if (ns <= 0) return 1;
    const int64_t ppb = ((ns + cap - 1) / cap + 255) / 256 * 256;
    return (int)((ns + ppb - 1) / ppb);
}
inline int nn_grid1(int64_t ns) { return icp_blocks(ns, 16384); }      // grid of the search kernel: one thread per point, capped
// the search kernel of one evaluation: per thread (27-cell block first where the correspondence distance spans two cells or more: blockf)
template <bool FROM_STATE>
void launch_icp_nn(gsr_icp_ctx* c, hipStream_t st, const Xform& X, const IcpState* state, double mc2, bool blockf) {
    const int g1 = nn_grid1(c->ns);
    const dim3 grid(8 * ((g1 + 7) / 8)), blk(256);
    const int nbl = c->xcd_ranges ? g1 : -g1;
    if (blockf)
        hipLaunchKernelGGL((k_icp_nn<FROM_STATE, 1>), grid, blk, 0, st, c->ns, c->src.as<float>(), X, state, c->index.grid, c->index.cellStart.as<int>(), c->index.Tq.as<float4>(), mc2,
                           c->nn_j.as<int>(), nbl);
    else
        hipLaunchKernelGGL((k_icp_nn<FROM_STATE, 0>), grid, blk, 0, st, c->ns, c->src.as<float>(), X, state, c->index.grid, c->index.cellStart.as<int>(), c->index.Tq.as<float4>(), mc2,
                           c->nn_j.as<int>(), nbl);
}

// The scaled estimator, checked on the arguments alone (before any context is looked at): with_scaling exists for point-to-point
// only (Open3D offers it nowhere else), and a robust loss does not apply to it -- kind 0 ignores the loss argument, the new kind
// says so.  Every other kind passes: what it needs is icp_check_kind's business.
int32_t icp_check_scaled(int kind, int loss, const char* who) {
    if (kind > GSR_ICP_POINT_TO_POINT_SCALED && kind <= (GSR_ICP_COLORED | GSR_ICP_WITH_SCALING))
        return fail(GSR_E_INVALID, "%s: with_scaling is offered for point-to-point estimation only (kind %d asks for it with kind %d)", who, kind,
                    kind & ~GSR_ICP_WITH_SCALING);
    if (kind == GSR_ICP_POINT_TO_POINT_SCALED && loss != GSR_LOSS_L2)
        return fail(GSR_E_INVALID, "%s: TransformationEstimationPointToPoint(with_scaling) takes no robust loss (loss %d)", who, loss);
    return GSR_OK;
}

// what an evaluation with estimator `kind` needs of the context
int32_t icp_check_kind(const gsr_icp_ctx* c, int kind) {
    if (!c->have_target || !c->have_source) return fail(GSR_E_INVALID, "icp: target and source must be set first");
    GSR_TRY(icp_check_scaled(kind, GSR_LOSS_L2, "icp"));
    if (kind < GSR_ICP_POINT_TO_POINT || kind > GSR_ICP_POINT_TO_POINT_SCALED) return fail(GSR_E_INVALID, "icp: unknown estimation kind %d", kind);
    if (kind == GSR_ICP_POINT_TO_PLANE && !c->have_normals)
        return fail(GSR_E_PRECONDITION, "TransformationEstimationPointToPlane requires target normals");
    if (kind == GSR_ICP_COLORED && (!c->have_normals || !c->have_tcol || !c->have_scol))
        return fail(GSR_E_PRECONDITION, "ColoredICP requires target normals and the colours of both clouds");
    if (kind == GSR_ICP_GENERALIZED && (!c->have_tcov || !c->have_scov))
        return fail(GSR_E_PRECONDITION, "TransformationEstimationForGeneralizedICP requires source and target covariances");
    return GSR_OK;
}

// one evaluation of the device-resident loop: 8 * ceil(nb / 8) workgroups, the padding ones get nothing (icp_block_range)
void launch_accumulate_dev(gsr_icp_ctx* c, hipStream_t st, int kind, bool blockf, int nb, const int* nnj, const ColorArgs& cargs, double mc2, int loss, double k) {
    const bool p2p = kind == GSR_ICP_POINT_TO_POINT || kind == GSR_ICP_POINT_TO_POINT_SCALED;
    const double* tn = p2p ? nullptr : (kind == GSR_ICP_GENERALIZED ? c->Tc.as<double>() : c->Tn.as<double>());
    const double* sc = kind == GSR_ICP_GENERALIZED ? c->Sc.as<double>() : nullptr;
    decltype(&k_icp_accumulate_dev<0, 0>) kernel = nullptr;
    switch (2 * kind + (blockf ? 1 : 0)) {
        case 0: kernel = k_icp_accumulate_dev<0, 0>; break;
        case 1: kernel = k_icp_accumulate_dev<0, 1>; break;
        case 2: kernel = k_icp_accumulate_dev<1, 0>; break;
        case 3: kernel = k_icp_accumulate_dev<1, 1>; break;
        case 4: kernel = k_icp_accumulate_dev<2, 0>; break;
        case 5: kernel = k_icp_accumulate_dev<2, 1>; break;
        case 6: kernel = k_icp_accumulate_dev<3, 0>; break;
        case 7: kernel = k_icp_accumulate_dev<3, 1>; break;
        case 8: kernel = k_icp_accumulate_dev<4, 0>; break;
        default: kernel = k_icp_accumulate_dev<4, 1>; break;
    }
    hipLaunchKernelGGL(kernel, dim3(8 * ((nb + 7) / 8)), dim3(256), 0, st, c->ns, c->src.as<float>(), c->state.as<IcpState>(), c->index.grid, c->index.cellStart.as<int>(), nnj,
                       c->index.Tq.as<float4>(), tn, sc, cargs, mc2, loss, k, c->partials.as<double>(), c->xcd_ranges ? nb : -nb);
}

int32_t run_accumulate(gsr_icp_ctx* c, const double* T, int kind, int loss, double k, double* acc, bool timed) {
    GSR_TRY(icp_check_kind(c, kind));
    hipStream_t st = c->stream;
    Xform X;
    for (int i = 0; i < 12; ++i) X.m[i] = T[i];
    const int nb = icp_blocks(c->ns, c->nblocks);
    GSR_TRY(c->partials.reserve((size_t)nb * GSR_ICP_ACC_LEN * 8));
    GSR_TRY(c->acc_dev.reserve(GSR_ICP_ACC_LEN * 8));
    GSR_HIP(hipMemsetAsync(c->partials.p, 0, (size_t)nb * GSR_ICP_ACC_LEN * 8, st));
    if (timed) GSR_HIP(hipEventRecord(c->e0, st));
    const double mc2 = c->max_corr * c->max_corr;
    const int* nnj = nullptr;
    if (c->nn_mode()) {
        GSR_TRY(c->nn_j.reserve((size_t)c->ns * 4));
        launch_icp_nn<false>(c, st, X, (const IcpState*)nullptr, mc2, false);
        nnj = c->nn_j.as<int>();
    }
    const ColorArgs cargs = {c->Ti.as<double>(), c->Tg.as<double>(), c->Si.as<double>(), sqrt(c->lambda_geometric), sqrt(1.0 - c->lambda_geometric)};
    if (kind == GSR_ICP_COLORED)
        hipLaunchKernelGGL(k_icp_accumulate<3>, dim3(nb), dim3(256), 0, st, c->ns, c->src.as<float>(), X, c->index.grid, c->index.cellStart.as<int>(), nnj,
                           c->index.Tq.as<float4>(), c->Tn.as<double>(), (const double*)nullptr, cargs, mc2, loss, k, c->partials.as<double>());
    else if (kind == GSR_ICP_POINT_TO_POINT)
        hipLaunchKernelGGL(k_icp_accumulate<0>, dim3(nb), dim3(256), 0, st, c->ns, c->src.as<float>(), X, c->index.grid, c->index.cellStart.as<int>(), nnj,
                           c->index.Tq.as<float4>(), (const double*)nullptr, (const double*)nullptr, cargs, mc2, loss, k, c->partials.as<double>());
    else if (kind == GSR_ICP_POINT_TO_POINT_SCALED)
        hipLaunchKernelGGL(k_icp_accumulate<4>, dim3(nb), dim3(256), 0, st, c->ns, c->src.as<float>(), X, c->index.grid, c->index.cellStart.as<int>(), nnj,
                           c->index.Tq.as<float4>(), (const double*)nullptr, (const double*)nullptr, cargs, mc2, loss, k, c->partials.as<double>());
    else if (kind == GSR_ICP_POINT_TO_PLANE)
        hipLaunchKernelGGL(k_icp_accumulate<1>, dim3(nb), dim3(256), 0, st, c->ns, c->src.as<float>(), X, c->index.grid, c->index.cellStart.as<int>(), nnj,
                           c->index.Tq.as<float4>(), c->Tn.as<double>(), (const double*)nullptr, cargs, mc2, loss, k, c->partials.as<double>());
    else
        hipLaunchKernelGGL(k_icp_accumulate<2>, dim3(nb), dim3(256), 0, st, c->ns, c->src.as<float>(), X, c->index.grid, c->index.cellStart.as<int>(), nnj,
                           c->index.Tq.as<float4>(), c->Tc.as<double>(), c->Sc.as<double>(), cargs, mc2, loss, k, c->partials.as<double>());
    hipLaunchKernelGGL(k_fold_partials<64>, dim3(GSR_ICP_ACC_LEN), dim3(64), 0, st, (int64_t)nb, GSR_ICP_ACC_LEN, (const double*)c->partials.as<double>(), c->acc_dev.as<double>());
    if (timed) GSR_HIP(hipEventRecord(c->e1, st));
    GSR_HIP(hipMemcpyAsync(acc, c->acc_dev.p, GSR_ICP_ACC_LEN * 8, hipMemcpyDeviceToHost, st));
    GSR_HIP(hipStreamSynchronize(st));
    if (timed) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->e0, c->e1);
        c->ms_iter += ms;
        c->n_iter_kernels += 1;
    }
    if (c->allreduce) {
        int32_t r = c->allreduce(acc, GSR_ICP_ACC_LEN, c->allreduce_user);
        if (r != 0) return fail(GSR_E_INVALID, "icp: all-reduce callback returned %d", r);
    }
    return GSR_OK;
}

}  // namespace

extern "C" {


int32_t gsr_icp_create(gsr_icp_ctx** out, int32_t device, void* stream) {
    if (!out) return fail(GSR_E_INVALID, "gsr_icp_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GSR_E_NO_DEVICE, "gsr_icp_create: no HIP device visible (this backend has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(GSR_E_INVALID, "gsr_icp_create: device %d out of range", device);
    GSR_HIP(hipSetDevice(device));
    gsr_icp_ctx* c = new gsr_icp_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;
    if (c->e0.create() != hipSuccess || c->e1.create() != hipSuccess || c->eb0.create() != hipSuccess || c->eb1.create() != hipSuccess) {
        delete c; return fail(GSR_E_HIP, "hipEventCreate failed");
    }
    // Environment knobs (the grid's own: GridIndex, csrc/grid.hip): none changes a result, tests/test_icp_gpu.py::test_icp_knobs_change_nothing
    if (const char* e = getenv("GSR_ICP_DEVICE_LOOP")) c->device_loop = atoi(e) != 0;
    if (const char* e = getenv("GSR_ICP_BLOCK_SEARCH")) c->block_search = atoi(e) != 0;
    if (const char* e = getenv("GSR_ICP_XCD")) c->xcd_ranges = atoi(e) != 0;
    if (const char* e = getenv("GSR_ICP_BLOCKS")) { int v = atoi(e); if (v >= 1 && v <= 65536) c->nblocks = v; }
    if (const char* e = getenv("GSR_ICP_NN_KERNEL")) c->nn_kernel = atoi(e);
    *out = c;
    return GSR_OK;
}

int32_t gsr_icp_destroy(gsr_icp_ctx* c) {
    delete c;       // (NULL: nothing)
    return GSR_OK;
}

int32_t gsr_icp_set_target(gsr_icp_ctx* c, const float* xyz, const double* normals, int64_t n, double max_corr, int32_t on_device) {
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_set_target: NULL context");
    if (!(max_corr > 0)) return fail(GSR_E_PRECONDITION, "max_correspondence_distance must be > 0 (got %g)", max_corr);
    if (n <= 0 || !xyz) return fail(GSR_E_PRECONDITION, "gsr_icp_set_target: empty target cloud");
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "gsr_icp_set_target: n too large");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GSR_HIP(hipEventRecord(c->eb0, st));
    const float* dxyz = xyz;
    const double* dnrm = normals;
    if (!on_device) {
        GSR_TRY(c->stage_xyz.reserve((size_t)n * 12));
        GSR_HIP(hipMemcpyAsync(c->stage_xyz.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
        dxyz = c->stage_xyz.as<float>();
        if (normals) {
            GSR_TRY(c->stage_nrm.reserve((size_t)n * 24));
            GSR_HIP(hipMemcpyAsync(c->stage_nrm.p, normals, (size_t)n * 24, hipMemcpyHostToDevice, st));
            dnrm = c->stage_nrm.as<double>();
        }
    }
    if (normals) GSR_TRY(c->Tn.reserve((size_t)n * 24));
    GSR_TRY(c->index.build(dxyz, n, max_corr, st, dnrm, c->Tn.as<double>()));
    GSR_HIP(hipEventRecord(c->eb1, st));
    if (c->defer_sync) c->build_pending = true;      // (gsr_icp_register_clouds: the registration behind this waits for the stream)
    else {
        GSR_HIP(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&c->ms_build, c->eb0, c->eb1);
        c->build_pending = false;
    }
    c->nt = n; c->max_corr = max_corr; c->have_target = true; c->have_normals = normals != nullptr;
    c->have_tcov = false; c->have_scov = false; c->have_tcol = false; c->have_scol = false;
    c->have_source = false;              // the source is sorted by the target grid: set it again after a new target
    return GSR_OK;
}

int32_t gsr_icp_set_source(gsr_icp_ctx* c, const float* xyz, int64_t n, int32_t on_device) {
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_set_source: NULL context");
    if (n < 0 || (n > 0 && !xyz)) return fail(GSR_E_PRECONDITION, "gsr_icp_set_source: empty source cloud");
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "gsr_icp_set_source: n too large");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    GSR_TRY(c->src.reserve((size_t)(n > 0 ? n : 1) * 12));
    c->src_sorted = false;
    if (n == 0) {
        // an empty shard of a multi-GPU source split (fewer points than ranks): it contributes zero sums and still joins
        // every collective; a registration without an all-reduce refuses it (gsr_icp_register)
    } else if (c->have_target) {
        // sort the source by the TARGET grid's cell (rigid motions keep neighbours neighbours): lanes of a
        // wave then walk the same target cells, and the per-point ring searches share cache lines
        const float* raw = xyz;                       // device arrays are read in place (this call returns synchronised)
        if (!on_device) {
            GSR_TRY(c->src_raw.reserve((size_t)n * 12));
            GSR_HIP(hipMemcpyAsync(c->src_raw.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
            raw = c->src_raw.as<float>();
        }
        GSR_TRY(c->index.sort_by_cell(raw, n, c->src_order, st));
        hipLaunchKernelGGL(k_icp_gather_source, dim3(stride_grid(n)), dim3(256), 0, st, n, c->src_order.as<unsigned>(), raw, c->src.as<float>());
        c->src_sorted = true;
    } else {
        GSR_HIP(hipMemcpyAsync(c->src.p, xyz, (size_t)n * 12, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    if (!c->defer_sync) GSR_HIP(hipStreamSynchronize(st));
    c->ns = n; c->have_source = true; c->have_scov = false; c->have_scol = false;
    if (!c->allreduce && !c->allreduce_dev && !c->comm) c->ns_global = n;
    return GSR_OK;
}

static int32_t set_cov(gsr_icp_ctx* c, const double* cov6, int64_t n, const unsigned* order, DevBuf& dst, int32_t on_device) {
    if (n == 0) return dst.reserve(48);               // an empty shard of a multi-GPU source split: nothing to gather
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const double* in = cov6;
    if (!on_device) {
        GSR_TRY(c->stage_cov.reserve((size_t)n * 48));
        GSR_HIP(hipMemcpyAsync(c->stage_cov.p, cov6, (size_t)n * 48, hipMemcpyHostToDevice, st));
        in = c->stage_cov.as<double>();
    }
    GSR_TRY(dst.reserve((size_t)n * 48));
    hipLaunchKernelGGL(k_icp_gather_cov, dim3(stride_grid(6 * n)), dim3(256), 0, st, n, order, in, dst.as<double>());
    GSR_HIP(hipStreamSynchronize(st));
    return GSR_OK;
}
int32_t gsr_icp_set_target_cov(gsr_icp_ctx* c, const double* cov6, int32_t on_device) {
    if (!c || !cov6) return fail(GSR_E_INVALID, "gsr_icp_set_target_cov: NULL argument");
    if (!c->have_target) return fail(GSR_E_PRECONDITION, "gsr_icp_set_target_cov: set the target first");
    GSR_TRY(set_cov(c, cov6, c->nt, c->index.order.as<unsigned>(), c->Tc, on_device));
    c->have_tcov = true;
    return GSR_OK;
}
int32_t gsr_icp_set_source_cov(gsr_icp_ctx* c, const double* cov6, int32_t on_device) {
    if (!c || (!cov6 && !(c->have_source && c->ns == 0))) return fail(GSR_E_INVALID, "gsr_icp_set_source_cov: NULL argument");
    if (!c->have_source) return fail(GSR_E_PRECONDITION, "gsr_icp_set_source_cov: set the source first");
    GSR_TRY(set_cov(c, cov6, c->ns, c->src_sorted ? c->src_order.as<unsigned>() : (const unsigned*)nullptr, c->Sc, on_device));
    c->have_scov = true;
    return GSR_OK;
}

int32_t gsr_icp_set_target_color(gsr_icp_ctx* c, const double* rgb, int32_t on_device) {
    if (!c || !rgb) return fail(GSR_E_INVALID, "gsr_icp_set_target_color: NULL argument");
    if (!c->have_target) return fail(GSR_E_PRECONDITION, "gsr_icp_set_target_color: set the target first");
    if (!c->have_normals) return fail(GSR_E_PRECONDITION, "ColoredICP requires pre-computed normal vectors for target PointCloud.");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t n = c->nt;
    const double* in = rgb;
    if (!on_device) {
        GSR_TRY(c->stage_cov.reserve((size_t)n * 24));
        GSR_HIP(hipMemcpyAsync(c->stage_cov.p, rgb, (size_t)n * 24, hipMemcpyHostToDevice, st));
        in = c->stage_cov.as<double>();
    }
    GSR_TRY(c->Ti.reserve((size_t)n * 8)); GSR_TRY(c->Tg.reserve((size_t)n * 24));
    hipLaunchKernelGGL(k_icp_intensity, dim3(stride_grid(n)), dim3(256), 0, st, n, c->index.order.as<unsigned>(), in, c->Ti.as<double>());
    // InitializePointCloudForColoredICP: KDTreeSearchParamHybrid(max_distance * 2, 30)
    hipLaunchKernelGGL(k_icp_color_gradient, dim3(stride_grid(n)), dim3(256), 0, st, n, c->index.grid, c->index.cellStart.as<int>(), c->index.Tq.as<float4>(),
                       c->Tn.as<double>(), c->Ti.as<double>(), c->max_corr * 2.0, c->Tg.as<double>());
    GSR_HIP(hipStreamSynchronize(st));
    c->have_tcol = true;
    return GSR_OK;
}
int32_t gsr_icp_set_source_color(gsr_icp_ctx* c, const double* rgb, int32_t on_device) {
    if (!c || (!rgb && !(c->have_source && c->ns == 0))) return fail(GSR_E_INVALID, "gsr_icp_set_source_color: NULL argument");
    if (!c->have_source) return fail(GSR_E_PRECONDITION, "gsr_icp_set_source_color: set the source first");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t n = c->ns;
    if (n == 0) { GSR_TRY(c->Si.reserve(8)); c->have_scol = true; return GSR_OK; }      // an empty shard of a multi-GPU source split
    const double* in = rgb;
    if (!on_device) {
        GSR_TRY(c->stage_cov.reserve((size_t)n * 24));
        GSR_HIP(hipMemcpyAsync(c->stage_cov.p, rgb, (size_t)n * 24, hipMemcpyHostToDevice, st));
        in = c->stage_cov.as<double>();
    }
    GSR_TRY(c->Si.reserve((size_t)n * 8));
    hipLaunchKernelGGL(k_icp_intensity, dim3(stride_grid(n)), dim3(256), 0, st, n, c->src_sorted ? c->src_order.as<unsigned>() : (const unsigned*)nullptr,
                       in, c->Si.as<double>());
    GSR_HIP(hipStreamSynchronize(st));
    c->have_scol = true;
    return GSR_OK;
}
int32_t gsr_icp_set_lambda_geometric(gsr_icp_ctx* c, double lambda_geometric) {
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_set_lambda_geometric: NULL context");
    if (!(lambda_geometric >= 0.0 && lambda_geometric <= 1.0)) return fail(GSR_E_INVALID, "lambda_geometric must lie in [0, 1]");
    c->lambda_geometric = lambda_geometric;
    return GSR_OK;
}
int32_t gsr_icp_get_color_gradient(gsr_icp_ctx* c, double* out) {
    if (!c || !out) return fail(GSR_E_INVALID, "gsr_icp_get_color_gradient: NULL argument");
    if (!c->have_tcol) return fail(GSR_E_PRECONDITION, "gsr_icp_get_color_gradient: set the target colours first");
    GSR_HIP(hipSetDevice(c->device));
    // back to the caller's point order (host memory)
    std::vector<double> sorted((size_t)c->nt * 3);
    std::vector<unsigned> order((size_t)c->nt);
    GSR_HIP(hipMemcpy(sorted.data(), c->Tg.p, (size_t)c->nt * 24, hipMemcpyDeviceToHost));
    GSR_HIP(hipMemcpy(order.data(), c->index.order.p, (size_t)c->nt * 4, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < c->nt; ++j)
        for (int a = 0; a < 3; ++a) out[3 * (size_t)order[j] + a] = sorted[3 * j + a];
    return GSR_OK;
}

int32_t gsr_icp_set_allreduce_dev(gsr_icp_ctx* c, gsr_allreduce_dev64_fn fn, void* user, int64_t n_source_global) {
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_set_allreduce_dev: NULL context");
    c->allreduce_dev = fn; c->allreduce_dev_user = user;
    if (fn) { c->allreduce = nullptr; c->allreduce_user = nullptr; c->comm = nullptr; }
    c->ns_global = fn ? n_source_global : c->ns;
    return GSR_OK;
}
int32_t gsr_icp_set_comm(gsr_icp_ctx* c, gsr_comm* comm, int64_t n_source_global) {
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_set_comm: NULL context");
    c->comm = comm;
    if (comm) { c->allreduce = nullptr; c->allreduce_user = nullptr; c->allreduce_dev = nullptr; c->allreduce_dev_user = nullptr; }
    c->ns_global = comm ? n_source_global : c->ns;
    return GSR_OK;
}
int32_t gsr_icp_set_allreduce(gsr_icp_ctx* c, gsr_allreduce_fn fn, void* user, int64_t n_source_global) {
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_set_allreduce: NULL context");
    c->allreduce = fn; c->allreduce_user = user;
    if (fn) { c->allreduce_dev = nullptr; c->allreduce_dev_user = nullptr; c->comm = nullptr; }
    c->ns_global = fn ? n_source_global : c->ns;
    return GSR_OK;
}

int32_t gsr_icp_accumulate(gsr_icp_ctx* c, const double* T, int32_t kind, int32_t loss, double k, double* acc) {
    GSR_TRY(icp_check_scaled(kind, loss, "gsr_icp_accumulate"));
    if (!c || !T || !acc) return fail(GSR_E_INVALID, "gsr_icp_accumulate: NULL argument");
    GSR_HIP(hipSetDevice(c->device));
    return run_accumulate(c, T, kind, loss, k, acc, false);
}

int32_t gsr_icp_register(gsr_icp_ctx* c, const double* init_T, int32_t kind, int32_t loss, double k, double rel_fitness,
                         double rel_rmse, int32_t max_iter, double* out_T, double* fitness, double* inlier_rmse, int32_t* iterations) {
    GSR_TRY(icp_check_scaled(kind, loss, "gsr_icp_register"));
    if (!c || !init_T || !out_T) return fail(GSR_E_INVALID, "gsr_icp_register: NULL argument");
    GSR_HIP(hipSetDevice(c->device));
    c->ms_iter = 0; c->n_iter_kernels = 0;
    const bool multi = c->allreduce_dev != nullptr || c->comm != nullptr;      // a device-side all-reduce per iteration
    if (!c->allreduce && !multi && c->have_source && c->ns == 0)
        return fail(GSR_E_PRECONDITION, "gsr_icp_register: empty source cloud");
    if (!c->allreduce && (c->device_loop || multi)) {
        // device-resident loop: no per-iteration host round trip.  With a device all-reduce (multi-GPU source split) the
        // only addition per iteration is one stream-ordered collective on 32 doubles between the reduction and the solve.
        GSR_TRY(icp_check_kind(c, kind));
        hipStream_t st = c->stream;
        IcpState hs;
        memset(&hs, 0, sizeof(hs));
        memcpy(hs.T, init_T, sizeof(hs.T));
        hs.ctr[0] = c->index.grid.cx; hs.ctr[1] = c->index.grid.cy; hs.ctr[2] = c->index.grid.cz;
        hs.nsg = (double)(multi ? c->ns_global : c->ns); hs.rel_fit = rel_fitness; hs.rel_rmse = rel_rmse;
        hs.max_iter = max_iter < 0 ? 0 : max_iter; hs.kind = kind;
        GSR_TRY(c->state.reserve(sizeof(IcpState)));
        GSR_HIP(hipMemcpyAsync(c->state.p, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
        const int nb = icp_blocks(c->ns, c->nblocks);
        GSR_TRY(c->partials.reserve((size_t)nb * GSR_ICP_ACC_LEN * 8));
        GSR_TRY(c->nn_j.reserve((size_t)(c->ns > 0 ? c->ns : 1) * 4));
        GSR_TRY(c->acc_dev.reserve(GSR_ICP_ACC_LEN * 8));
        GSR_HIP(hipMemsetAsync(c->partials.p, 0, (size_t)nb * GSR_ICP_ACC_LEN * 8, st));
        const double mc2 = c->max_corr * c->max_corr;
        const ColorArgs cargs = {c->Ti.as<double>(), c->Tg.as<double>(), c->Si.as<double>(), sqrt(c->lambda_geometric), sqrt(1.0 - c->lambda_geometric)};
        const int total_evals = hs.max_iter + 1;
        // the first 27 cells of the search as one block of batched loads when max_corr spans two or more cells (icp_nearest)
        const bool blockf = c->block_search && c->index.grid.rings >= 2;
        int issued = 0;
        GSR_HIP(hipEventRecord(c->e0, st));
        while (issued < total_evals) {
            const int chunk = total_evals - issued < 8 ? total_evals - issued : 8;
            const int* nnj = c->nn_mode() ? c->nn_j.as<int>() : (const int*)nullptr;
            for (int i = 0; i < chunk; ++i) {
                if (c->nn_mode()) launch_icp_nn<true>(c, st, Xform(), c->state.as<IcpState>(), mc2, blockf);
                launch_accumulate_dev(c, st, kind, blockf, nb, nnj, cargs, mc2, loss, k);
                if (multi) {
                    hipLaunchKernelGGL(k_icp_reduce, dim3(1), dim3(1024), 0, st, nb, c->partials.as<double>(), c->state.as<IcpState>(), c->acc_dev.as<double>());
                    if (c->comm) {                            // RCCL enqueued on this stream: no host involvement
                        GSR_TRY(gsr_comm_allreduce(c->comm, c->acc_dev.p, GSR_ICP_ACC_LEN, GSR_DT_F64, GSR_OP_SUM, (void*)st));
                    } else {
                        const int32_t rc = c->allreduce_dev(c->acc_dev.p, GSR_ICP_ACC_LEN, c->allreduce_dev_user);
                        if (rc != 0) return fail(GSR_E_INVALID, "icp: device all-reduce callback returned %d", rc);
                    }
                    hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(ICP_STEP_THREADS), 0, st, nb, c->partials.as<double>(), c->acc_dev.as<double>(), c->state.as<IcpState>());
                } else {
                    hipLaunchKernelGGL(k_icp_step, dim3(1), dim3(ICP_STEP_THREADS), 0, st, nb, c->partials.as<double>(), (const double*)nullptr, c->state.as<IcpState>());
                }
            }
            issued += chunk;
            GSR_HIP(hipGetLastError());              // a failed launch of the chunk (configuration, LDS) is reported here, not as a hang
            GSR_TRY(c->index.fetch(st, c->state.p, &hs, sizeof(hs)));
            if (hs.done) break;
        }
        GSR_HIP(hipEventRecord(c->e1, st));
        GSR_HIP(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&c->ms_iter, c->e0, c->e1);
        c->n_iter_kernels = hs.evals;
        memcpy(out_T, hs.T, sizeof(hs.T));
        if (fitness) *fitness = hs.fit;
        if (inlier_rmse) *inlier_rmse = hs.rmse;
        if (iterations) *iterations = hs.iters;
        return GSR_OK;
    }
    double T[16], acc[GSR_ICP_ACC_LEN], update[16];
    memcpy(T, init_T, sizeof(T));
    GSR_TRY(run_accumulate(c, T, kind, loss, k, acc, true));
    const double nsg = (double)(c->ns_global > 0 ? c->ns_global : c->ns);
    double fit = acc[0] > 0 ? acc[0] / nsg : 0.0, rmse = acc[0] > 0 ? sqrt(acc[1] / acc[0]) : 0.0;
    int it = 0;
    for (; it < max_iter; ++it) {
        const double ctr[3] = {c->index.grid.cx, c->index.grid.cy, c->index.grid.cz};
        estimate_update(ctr, kind, acc, update);
        mat4_mul(update, T, T);
        GSR_TRY(run_accumulate(c, T, kind, loss, k, acc, true));
        const double fit2 = acc[0] > 0 ? acc[0] / nsg : 0.0, rmse2 = acc[0] > 0 ? sqrt(acc[1] / acc[0]) : 0.0;
        const bool stop = fabs(fit - fit2) < rel_fitness && fabs(rmse - rmse2) < rel_rmse;
        fit = fit2; rmse = rmse2;
        if (stop) { ++it; break; }
    }
    memcpy(out_T, T, sizeof(T));
    if (fitness) *fitness = fit;
    if (inlier_rmse) *inlier_rmse = rmse;
    if (iterations) *iterations = it;
    return GSR_OK;
}

int32_t gsr_icp_correspondences(gsr_icp_ctx* c, const double* T, int64_t* idx, double* d2) {
    if (!c || !T || !idx || !d2) return fail(GSR_E_INVALID, "gsr_icp_correspondences: NULL argument");
    if (!c->have_target || !c->have_source) return fail(GSR_E_INVALID, "icp: target and source must be set first");
    GSR_HIP(hipSetDevice(c->device));
    GSR_TRY(c->corr_idx.reserve((size_t)c->ns * 8)); GSR_TRY(c->corr_d2.reserve((size_t)c->ns * 8));
    Xform X;
    for (int i = 0; i < 12; ++i) X.m[i] = T[i];
    GSR_TRY(c->nn_j.reserve((size_t)c->ns * 4));
    launch_icp_nn<false>(c, c->stream, X, (const IcpState*)nullptr, c->max_corr * c->max_corr, false);
    hipLaunchKernelGGL(k_icp_correspond, dim3(stride_grid(c->ns)), dim3(256), 0, c->stream, c->ns, c->src.as<float>(), X, c->nn_j.as<int>(),
                       c->index.Tq.as<float4>(), c->src_sorted ? c->src_order.as<unsigned>() : (const unsigned*)nullptr, c->corr_idx.as<int64_t>(),
                       c->corr_d2.as<double>());
    GSR_HIP(hipMemcpyAsync(idx, c->corr_idx.p, (size_t)c->ns * 8, hipMemcpyDeviceToHost, c->stream));
    GSR_HIP(hipMemcpyAsync(d2, c->corr_d2.p, (size_t)c->ns * 8, hipMemcpyDeviceToHost, c->stream));
    GSR_HIP(hipStreamSynchronize(c->stream));
    return GSR_OK;
}

int32_t gsr_icp_information(gsr_icp_ctx* c, const double* T, double* info36, int64_t* n_corr) {
    if (!c || !T || !info36) return fail(GSR_E_INVALID, "gsr_icp_information: NULL argument");
    if (!c->have_target || !c->have_source) return fail(GSR_E_INVALID, "gsr_icp_information: target and source must be set first");
    if (c->comm || c->allreduce || c->allreduce_dev)
        return fail(GSR_E_INVALID, "gsr_icp_information: one process, one GPU -- this context has a communicator or an all-reduce callback installed "
                                   "(the sums of a source shard are not the pair's information matrix)");
    for (int i = 0; i < 16; ++i)
        if (!(fabs(T[i]) <= DBL_MAX)) return fail(GSR_E_INVALID, "gsr_icp_information: T[%d] is not finite", i);
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    Xform X;
    for (int i = 0; i < 12; ++i) X.m[i] = T[i];
    const int nb = icp_blocks(c->ns, c->nblocks);
    GSR_TRY(c->partials.reserve((size_t)nb * GSR_ICP_ACC_LEN * 8));
    GSR_TRY(c->acc_dev.reserve(GSR_ICP_ACC_LEN * 8));
    GSR_HIP(hipMemsetAsync(c->partials.p, 0, (size_t)nb * GSR_ICP_ACC_LEN * 8, st));
    const double mc2 = c->max_corr * c->max_corr;
    const int* nnj = nullptr;
    if (c->nn_mode()) {                             // the search an evaluation of this context would take (run_accumulate)
        GSR_TRY(c->nn_j.reserve((size_t)c->ns * 4));
        launch_icp_nn<false>(c, st, X, (const IcpState*)nullptr, mc2, false);
        nnj = c->nn_j.as<int>();
    }
    hipLaunchKernelGGL(k_icp_information, dim3(nb), dim3(256), 0, st, c->ns, c->src.as<float>(), X, c->index.grid, c->index.cellStart.as<int>(), nnj, c->index.Tq.as<float4>(),
                       mc2, c->partials.as<double>());
    hipLaunchKernelGGL(k_fold_partials<64>, dim3(ICP_INFO_NACC), dim3(64), 0, st, (int64_t)nb, GSR_ICP_ACC_LEN, (const double*)c->partials.as<double>(), c->acc_dev.as<double>());
    double a[ICP_INFO_NACC];
    GSR_HIP(hipMemcpyAsync(a, c->acc_dev.p, sizeof(a), hipMemcpyDeviceToHost, st));
    GSR_HIP(hipStreamSynchronize(st));
    // Lambda = [[tr(S) I - S, [m]x], [[m]x^T, n I]]  with  n = a[0], m = sum q = a[1..3], S = sum q q^T = a[4..9] (xx xy xz yy yz zz)
    const double n = a[0], mx = a[1], my = a[2], mz = a[3];
    const double nxy = 0.0 - a[5], nxz = 0.0 - a[6], nyz = 0.0 - a[8];                 // 0.0 - x: no negative zeros in an empty matrix
    const double A[3][3] = {{a[7] + a[9], nxy, nxz}, {nxy, a[4] + a[9], nyz}, {nxz, nyz, a[4] + a[7]}};      // tr(S) I - S
    const double Mx[3][3] = {{0.0, 0.0 - mz, my}, {mz, 0.0, 0.0 - mx}, {0.0 - my, mx, 0.0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            info36[6 * i + j] = A[i][j];
            info36[6 * i + 3 + j] = Mx[i][j];
            info36[6 * (3 + i) + j] = Mx[j][i];
            info36[6 * (3 + i) + 3 + j] = i == j ? n : 0.0;
        }
    if (n_corr) *n_corr = (int64_t)n;
    return GSR_OK;
}

int32_t gsr_icp_solve(const double* acc, int32_t kind, const double* centre, double* update) {
    if (!acc || !update) return fail(GSR_E_INVALID, "gsr_icp_solve: NULL argument");
    GSR_TRY(icp_check_scaled(kind, GSR_LOSS_L2, "gsr_icp_solve"));
    if (kind < GSR_ICP_POINT_TO_POINT || kind > GSR_ICP_POINT_TO_POINT_SCALED) return fail(GSR_E_INVALID, "gsr_icp_solve: unknown kind %d", kind);
    const double zero[3] = {0, 0, 0};
    estimate_update(centre ? centre : zero, kind, acc, update);
    return GSR_OK;
}

int32_t gsr_icp_get_centre(gsr_icp_ctx* c, double* centre3) {
    if (!c || !centre3 || !c->have_target) return fail(GSR_E_INVALID, "gsr_icp_get_centre: no target set");
    centre3[0] = c->index.grid.cx; centre3[1] = c->index.grid.cy; centre3[2] = c->index.grid.cz;
    return GSR_OK;
}

static void icp_read_build_ms(gsr_icp_ctx* c) {
    if (!c->build_pending) return;
    (void)hipEventSynchronize(c->eb1);
    (void)hipEventElapsedTime(&c->ms_build, c->eb0, c->eb1);
    c->build_pending = false;
}

// registration_icp(source, target, max_correspondence_distance, init, estimation, criteria) -- Open3D's own entry takes the two CLOUDS
// (local_registration_util.py:88-90): target index, source order and the iteration loop in one call, no return to the host language and
// no stream synchronisation between them (a Python caller spent ~0.2 ms per registration in those gaps: profiles/r06d_icp_timeline.txt).
int32_t gsr_icp_register_clouds(gsr_icp_ctx* c, const float* src_xyz, int64_t ns, const float* tgt_xyz, const double* tgt_normals, int64_t nt,
                                int32_t on_device, double max_corr, const double* init_T, int32_t kind, int32_t loss, double k, double rel_fitness,
                                double rel_rmse, int32_t max_iter, double* out_T, double* fitness, double* inlier_rmse, int32_t* iterations) {
    GSR_TRY(icp_check_scaled(kind, loss, "gsr_icp_register_clouds"));
    if (!c) return fail(GSR_E_INVALID, "gsr_icp_register_clouds: NULL context");
    if (kind != GSR_ICP_POINT_TO_POINT && kind != GSR_ICP_POINT_TO_PLANE && kind != GSR_ICP_POINT_TO_POINT_SCALED)
        return fail(GSR_E_INVALID, "gsr_icp_register_clouds: point-to-point and point-to-plane only (covariances / colours: the step-by-step entry points)");
    if (kind == GSR_ICP_POINT_TO_PLANE && !tgt_normals) return fail(GSR_E_PRECONDITION, "TransformationEstimationPointToPlane requires target normals");
    // one process, one GPU: a communicator or an all-reduce callback of an earlier sharded call must not stay behind
    c->comm = nullptr; c->allreduce = nullptr; c->allreduce_user = nullptr; c->allreduce_dev = nullptr; c->allreduce_dev_user = nullptr;
    c->defer_sync = c->device_loop;                 // (the host-driven loop, GSR_ICP_DEVICE_LOOP=0, keeps the waits)
    int32_t r = gsr_icp_set_target(c, tgt_xyz, kind == GSR_ICP_POINT_TO_PLANE ? tgt_normals : nullptr, nt, max_corr, on_device);
    if (r == GSR_OK) r = gsr_icp_set_source(c, src_xyz, ns, on_device);
    c->defer_sync = false;
    if (r == GSR_OK) { c->ns_global = ns; r = gsr_icp_register(c, init_T, kind, loss, k, rel_fitness, rel_rmse, max_iter, out_T, fitness, inlier_rmse, iterations); }
    if (r != GSR_OK) (void)hipStreamSynchronize(c->stream);         // (the caller's arrays are free again whatever happened)
    icp_read_build_ms(c);
    return r;
}

// The coarse-to-fine schedule in one call (MultiScaleRegistratorMixture._register_main_point_clouds, qt_multiscale_registrator.py:197-236: entry k registers
// level list[-(k + 1)] of the two clouds from the transform entry k - 1 ended with): gsr_icp_register_clouds per entry, no return to the host language between
// the entries.  entries[k] describes entry k (coarsest first); results[k] receives its outcome; out_T the last entry's transform.
int32_t gsr_icp_register_multiscale(gsr_icp_ctx* c, int32_t n_entries, const gsr_icp_entry* entries, int32_t on_device, const double* init_T, int32_t kind,
                                    int32_t loss, double k, double rel_fitness, double rel_rmse, gsr_icp_entry_result* results, double* out_T) {
    GSR_TRY(icp_check_scaled(kind, loss, "gsr_icp_register_multiscale"));
    if (!c || !init_T || !out_T || n_entries < 0 || (n_entries > 0 && (!entries || !results)))
        return fail(GSR_E_INVALID, "gsr_icp_register_multiscale: bad argument");
    double T[16];
    memcpy(T, init_T, sizeof(T));
    for (int e = 0; e < n_entries; ++e) {
        const gsr_icp_entry& E = entries[e];
        gsr_icp_entry_result& R = results[e];
        memset(&R, 0, sizeof(R));
        memcpy(R.init_T, T, sizeof(T));
        const int32_t r = gsr_icp_register_clouds(c, E.src_xyz, E.ns, E.tgt_xyz, E.tgt_normals, E.nt, on_device, E.max_corr, T, kind, loss, k, rel_fitness, rel_rmse,
                                                  E.max_iter, R.T, &R.fitness, &R.inlier_rmse, &R.iterations);
        if (r != GSR_OK) return r;
        R.ms_build = c->ms_build; R.ms_iters = c->ms_iter; R.evaluations = c->n_iter_kernels;
        memcpy(T, R.T, sizeof(T));
    }
    memcpy(out_T, T, sizeof(T));
    return GSR_OK;
}

int32_t gsr_icp_get_timing(gsr_icp_ctx* c, float* out3) {
    if (!c || !out3) return fail(GSR_E_INVALID, "gsr_icp_get_timing: NULL argument");
    icp_read_build_ms(c);
    out3[0] = c->ms_build; out3[1] = c->ms_iter; out3[2] = (float)c->n_iter_kernels;
    return GSR_OK;
}

int32_t gsr_normals_from_cov(const float* cov6, int64_t n, double* normals, int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!cov6 || !normals))) return fail(GSR_E_INVALID, "gsr_normals_from_cov: bad argument");
    GSR_TRY(open_device(device, "gsr_normals_from_cov"));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_normals_from_cov");
    const float* in = nullptr;
    double* out = nullptr;
    GSR_TRY(os.in(cov6, (size_t)n * 24, &in));
    GSR_TRY(os.out(normals, (size_t)n * 24, &out));
    hipLaunchKernelGGL(k_normals_from_cov, dim3(stride_grid(n)), dim3(256), 0, os.st, n, in, out);
    return os.finish();
}

int32_t gsr_cov_from_normals(const double* normals, int64_t n, double epsilon, double* cov6, int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!normals || !cov6))) return fail(GSR_E_INVALID, "gsr_cov_from_normals: bad argument");
    GSR_TRY(open_device(device, "gsr_cov_from_normals"));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_cov_from_normals");
    const double* in = nullptr;
    double* out = nullptr;
    GSR_TRY(os.in(normals, (size_t)n * 24, &in));
    GSR_TRY(os.out(cov6, (size_t)n * 48, &out));
    hipLaunchKernelGGL(k_cov_from_normals, dim3(stride_grid(n)), dim3(256), 0, os.st, n, in, epsilon, out);
    return os.finish();
}

// test hook (gsr_test_hooks.h): the two stages of gsr_fold.h on caller-supplied rows
int32_t gsr_debug_fold(const double* x, int64_t n, int32_t order, int32_t final_threads, double* out3, int32_t device) {
    if (n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && !x) || !out3 || (order != 0 && order != 1) || (final_threads != 64 && final_threads != 256))
        return fail(GSR_E_INVALID, "gsr_debug_fold: bad argument");
    GSR_TRY(open_device(device, "gsr_debug_fold"));
    out3[0] = out3[1] = out3[2] = 0.0;
    if (n == 0) return GSR_OK;
    OneShot os(nullptr, false, "gsr_debug_fold");
    const int nb = (int)((n + 255) / 256);
    const double* dx = nullptr;
    double *partials = nullptr, *dout = nullptr;
    GSR_TRY(os.in(x, (size_t)n * 24, &dx));
    GSR_TRY(os.scratch((size_t)nb * 4 * 8, &partials));
    GSR_TRY(os.out(out3, 3 * 8, &dout));
    if (order == 0) hipLaunchKernelGGL(k_debug_fold<wave_sum_xor>, dim3(nb), dim3(256), 0, os.st, n, dx, partials);
    else hipLaunchKernelGGL(k_debug_fold<wave_sum_rows>, dim3(nb), dim3(256), 0, os.st, n, dx, partials);
    if (final_threads == 64) hipLaunchKernelGGL(k_fold_partials<64>, dim3(3), dim3(64), 0, os.st, (int64_t)nb, 4, (const double*)partials, dout);
    else hipLaunchKernelGGL(k_fold_partials<256>, dim3(3), dim3(256), 0, os.st, (int64_t)nb, 4, (const double*)partials, dout);
    return os.finish();
}

}  // extern "C"
