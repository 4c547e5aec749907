// clean.hip -- floater removal (gsr_outlier_mask) and row selection (gsr_model_select), include/gsr_hip.h; DESIGN.md section 18.
//
//   k_clean_prep                 finite test and the two splat gates; the search copy of xyz with every dropped row NaNed out
//   GridIndex::build             the point grid over that copy (csrc/grid.hip: robust box, cell-sorted float4 with the input index)
//   k_knn_mean<KMAX>             a lane per cell-sorted query: the KMAX smallest d^2 in registers (compile-time indices only), the
//                                expanding-ring walk (its own copy of grid_ring_walk) capped at CLEAN_RING_CAP rings; what has not met
//                                its stop rule by then goes to a list (ballot compaction, one integer atomic per wave)
//   k_knn_mean_deferred          a wave per listed query: (y, z) rows outward until k' candidates are known, then ONE pass over the
//                                bounds of all other rows against the k'-th best, rows scanned 64 points at a time (wave_scan_take)
//   k_clean_moment / _final x2   cloud_mean, then the squared deviations: per-block partials, combined in block order
//   k_clean_stat                 the statistical verdict; a dropped row is NaNed out of the sorted points
//   k_radius_count               strict count within radius^2 over grid_box_walk's ceil(radius / cell) + 1 rings of the same grid
//   k_clean_mask                 mask and the per-stage counts
//   k_select_flags / scan / k_select_index / k_model_select      kept-index list, then a lane per output float, one launch per array
//
// One stream, the kernel boundary is the only synchronisation.  No float atomics: the same input gives the same bits.
#include "gsr_clean_args.h"
#include "gsr_common.h"
#include "gsr_grid.h"
#include "gsr_oneshot.h"
#include "gsr_prims.h"

#include <float.h>
#include <math.h>

namespace gsr {

#define CLEAN_RING_CAP 3          // rings 0..3 of a lane's walk: 343 cells at about two points each
#define CLEAN_MOM_BLOCKS 1024     // most partials of a moment (the count is min(ceil(n / 256), this): a function of n alone)
// stage[i]: why row i was dropped (0: alive)
#define CLEAN_NONFINITE 1
#define CLEAN_GATE_OPACITY 2
#define CLEAN_GATE_SCALE 3
#define CLEAN_STATISTICAL 4
#define CLEAN_RADIUS 5
// counters (unsigned long long): rows dropped by stage 1..5 at [stage - 1], alive after the gates, kept, deferred queries
#define CLEAN_CTR_ALIVE 5
#define CLEAN_CTR_KEPT 6
#define CLEAN_CTR_DEFERRED 7
#define CLEAN_NCTR 8

__global__ __launch_bounds__(256) void k_clean_prep(int64_t n, const float* __restrict__ xyz, const float* __restrict__ op, const float* __restrict__ sc,
                                                    double min_op, double max_ls, float* __restrict__ sxyz, uint8_t* __restrict__ stage,
                                                    double* __restrict__ mean_out, int* __restrict__ count_out, unsigned long long* __restrict__ ctr) {
    const float nanv = __int_as_float(0x7fc00000);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        int s = 0;
        if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX)) s = CLEAN_NONFINITE;
        else if (op && !((double)op[i] >= min_op)) s = CLEAN_GATE_OPACITY;
        else if (sc && !((double)sc[3 * i] <= max_ls && (double)sc[3 * i + 1] <= max_ls && (double)sc[3 * i + 2] <= max_ls)) s = CLEAN_GATE_SCALE;
        stage[i] = (uint8_t)s;
        sxyz[3 * i] = s ? nanv : x; sxyz[3 * i + 1] = s ? nanv : y; sxyz[3 * i + 2] = s ? nanv : z;
        if (mean_out) mean_out[i] = -1.0;
        if (count_out) count_out[i] = -1;
        wave_count(s == CLEAN_NONFINITE, ctr + CLEAN_NONFINITE - 1);
        wave_count(s == CLEAN_GATE_OPACITY, ctr + CLEAN_GATE_OPACITY - 1);
        wave_count(s == CLEAN_GATE_SCALE, ctr + CLEAN_GATE_SCALE - 1);
        wave_count(s == 0, ctr + CLEAN_CTR_ALIVE);
    }
}

// mean_s[j] for the cell-sorted point j: the mean of the k' smallest distances (self included), -1 for a row that is out of the
// search.  The list is KMAX float64 in registers, kept ascending by an unrolled compare-exchange chain -- no index into it is a
// runtime value (an indexed array of this size lives in scratch: k_knn_normals).  `worst` is its k'-th entry: a candidate enters
// only below it.  Ties among equal distances cannot change the sum, so no index is kept.  The ring walk is grid_ring_walk's (gsr_grid.h),
// spelled out here: through the shared template the point loop measured 1.2 % slower where a lane scans a crowded boundary cell
// (DESIGN.md 6a), and this is the loop a cloud with many floaters spends its time in.
template <int KMAX>
__global__ __launch_bounds__(256) void k_knn_mean(int64_t nt, IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq, int knn,
                                                  const unsigned long long* __restrict__ ctr, double* __restrict__ mean_s,
                                                  int* __restrict__ deferred, unsigned long long* __restrict__ ndef) {
    const int64_t jq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool defer = false;
    if (jq < nt) {
        const float4 qv = Tq[jq];
        const double px = (double)qv.x, py = (double)qv.y, pz = (double)qv.z;
        double mean = -1.0;
        if (px == px && py == py && pz == pz) {
            const unsigned long long alive = ctr[CLEAN_CTR_ALIVE];
            const int kp = alive < (unsigned long long)knn ? (int)alive : knn;
            double kd[KMAX];
#pragma unroll
            for (int t = 0; t < KMAX; ++t) kd[t] = 1.0 / 0.0;
            double worst = 1.0 / 0.0;
            bool done = false;
            const int cx = icp_cell(px, g.ox, g.inv_c, g.gx), cy = icp_cell(py, g.oy, g.inv_c, g.gy), cz = icp_cell(pz, g.oz, g.inv_c, g.gz);
            const double eps = 1e-13 * (fabs(px) + fabs(py) + fabs(pz) + fabs(g.ox) + fabs(g.oy) + fabs(g.oz) + g.c * (double)(g.gx + g.gy + g.gz));
            for (int r = 0; r <= CLEAN_RING_CAP && !done; ++r) {
                for (int dz = -r; dz <= r; ++dz) {
                    const int z = cz + dz;
                    if (z < 0 || z >= g.gz) continue;
                    const int adz = dz < 0 ? -dz : dz;
                    for (int dy = -r; dy <= r; ++dy) {
                        const int y = cy + dy;
                        if (y < 0 || y >= g.gy) continue;
                        const int ady = dy < 0 ? -dy : dy;
                        const int rowbase = (z * g.gy + y) * g.gx;
                        const bool face = adz == r || ady == r;      // a face row of the ring: the whole x span; else the two end cells
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
                                const double d2 = dx * dx + dy2 * dy2 + dz2 * dz2;
                                if (d2 < worst) {                      // (NaN: a row that is out of the search)
                                    double v = d2;
#pragma unroll
                                    for (int t = 0; t < KMAX; ++t) {
                                        const bool sw = v < kd[t];
                                        const double lo = sw ? v : kd[t];
                                        v = sw ? kd[t] : v;
                                        kd[t] = lo;
                                    }
#pragma unroll
                                    for (int t = 0; t < KMAX; ++t) worst = t == kp - 1 ? kd[t] : worst;
                                }
                            }
                        }
                    }
                }
                // an unseen point lies at least `reach` away: done when the list is full (worst is finite) and its k'-th entry is strictly closer
                double reach = 1.0 / 0.0;
                if (cx - r > 0) reach = fmin(reach, px - (g.ox + (double)(cx - r) * g.c));
                if (cx + r < g.gx - 1) reach = fmin(reach, (g.ox + (double)(cx + r + 1) * g.c) - px);
                if (cy - r > 0) reach = fmin(reach, py - (g.oy + (double)(cy - r) * g.c));
                if (cy + r < g.gy - 1) reach = fmin(reach, (g.oy + (double)(cy + r + 1) * g.c) - py);
                if (cz - r > 0) reach = fmin(reach, pz - (g.oz + (double)(cz - r) * g.c));
                if (cz + r < g.gz - 1) reach = fmin(reach, (g.oz + (double)(cz + r + 1) * g.c) - pz);
                reach = reach * 0.999999999 - eps;
                if (reach > 0.0 && worst < reach * reach) done = true;
            }
            if (done) {
                double s = 0.0;
#pragma unroll
                for (int t = 0; t < KMAX; ++t)
                    if (t < kp) s += sqrt(kd[t]);
                mean = s / (double)kp;
            } else {
                defer = true;
            }
        }
        if (!defer) mean_s[jq] = mean;
    }
    const unsigned long long m = __ballot(defer);
    if (m) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(ndef, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (defer) deferred[base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = (int)jq;
    }
}

// One wave per deferred query.  Candidates go to an LDS list by ballot and are cut to the k' best by rank (hyb_rank_cut; the keys
// (d^2, input index) are unique) whenever the list would overflow and after every 64 rows.  First the (y, z) rows in square rings
// around the query's own row, each over its whole x span, until k' candidates are known; then one pass over ALL other rows, a lane
// per row: a row whose slab is strictly farther than the k'-th best is skipped, the others are clipped in x and scanned 64 points at
// a time.  A far floater thus costs the rows' bounds (two loads and a dozen flops each, 64 at a time) plus the points within its
// k'-th distance -- not every point on one lane.
__global__ __launch_bounds__(64) void k_knn_mean_deferred(IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq, int knn,
                                                          const unsigned long long* __restrict__ ctr, const int* __restrict__ deferred,
                                                          double* __restrict__ mean_s) {
    __shared__ double sd[GSR_HYBRID_CAP];
    __shared__ unsigned si[GSR_HYBRID_CAP];
    const int lane = threadIdx.x;
    const unsigned long long alive = ctr[CLEAN_CTR_ALIVE];
    const int kp = alive < (unsigned long long)knn ? (int)alive : knn;
    const long long nd = (long long)ctr[CLEAN_CTR_DEFERRED];
    for (long long qd = blockIdx.x; qd < nd; qd += gridDim.x) {
        const int jq = deferred[qd];
        const float4 qv = Tq[jq];
        const double px = (double)qv.x, py = (double)qv.y, pz = (double)qv.z;
        const int cy = icp_cell(py, g.oy, g.inv_c, g.gy), cz = icp_cell(pz, g.oz, g.inv_c, g.gz);
        const double eps = 1e-13 * (fabs(px) + fabs(py) + fabs(pz) + fabs(g.ox) + fabs(g.oy) + fabs(g.oz) + g.c * (double)(g.gx + g.gy + g.gz));
        int cnt = 0;
        double kth = 1.0 / 0.0;
        // the points [s0, e0) of the sorted array, 64 at a time (wave-uniform arguments)
        auto scan = [&](int s0, int e0) {                                  // (overflow: cnt > CAP - 64 >= k', the cut leaves exactly k')
            wave_scan_take(Tq, s0, e0, px, py, pz, sd, si, cnt, kp, [&](double d2, unsigned) { return d2 < kth; },      // (NaN: a row that is out of the search)
                           [&]() { kth = sd[kp - 1]; });
        };
        // the rows a lane flagged, one after the other
        auto scan_rows = [&](bool need, int s0, int e0) {
            unsigned long long m = __ballot(need);
            while (m) {
                const int b = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                scan(__shfl(s0, b), __shfl(e0, b));
            }
        };
        // ---- seed: square rings of rows around (cy, cz), whole x spans, until k' candidates are known or every row has been seen
        int ry = cy > g.gy - 1 - cy ? cy : g.gy - 1 - cy, rz = cz > g.gz - 1 - cz ? cz : g.gz - 1 - cz;
        const int rmax = ry > rz ? ry : rz;
        int rs = 0;
        for (;; ++rs) {
            const int side = 2 * rs + 1, nrows = rs == 0 ? 1 : 8 * rs;
            for (int t0 = 0; t0 < nrows; t0 += 64) {
                const int t = t0 + lane;
                int dy = 0, dz = 0;
                if (rs > 0) {
                    if (t < side) { dz = -rs; dy = t - rs; }
                    else if (t < 2 * side) { dz = rs; dy = t - side - rs; }
                    else if (t < 2 * side + side - 2) { dy = -rs; dz = t - 2 * side - rs + 1; }
                    else { dy = rs; dz = t - 2 * side - (side - 2) - rs + 1; }
                }
                const int y = cy + dy, z = cz + dz;
                const bool ok = t < nrows && y >= 0 && y < g.gy && z >= 0 && z < g.gz;
                const int rowbase = ok ? (z * g.gy + y) * g.gx : 0;
                const int s0 = ok ? cellStart[rowbase] : 0, e0 = ok ? cellStart[rowbase + g.gx] : 0;
                scan_rows(ok && e0 > s0, s0, e0);
            }
            if (cnt >= kp || rs >= rmax) break;
        }
        if (cnt >= kp) { cnt = hyb_rank_cut(sd, si, cnt, kp, nullptr); kth = sd[kp - 1]; }      // (sorted: the k'-th best is the last)
        // ---- every row outside the seed square, by its bound
        if (rs < rmax) {
            const int nyz = g.gy * g.gz;
            for (int t0 = 0; t0 < nyz; t0 += 64) {
                const int t = t0 + lane;
                bool need = false;
                int s0 = 0, e0 = 0;
                if (t < nyz) {
                    const int z = t / g.gy, y = t - z * g.gy;
                    const int ady = y > cy ? y - cy : cy - y, adz = z > cz ? z - cz : cz - z;
                    if (ady > rs || adz > rs) {
                        const double dyb = icp_slab_dist(py, g.oy, g.c, y, eps, g.gy), dzb = icp_slab_dist(pz, g.oz, g.c, z, eps, g.gz);
                        const double rem = kth - dyb * dyb - dzb * dzb;
                        if (rem >= 0.0) {                              // clip the x span to |dx| <= sqrt(rem), as icp_nearest does
                            const double hx = sqrt(rem) * 1.0001 + eps + 1e-30;
                            const int xlo = icp_cell(px - hx, g.ox, g.inv_c, g.gx), xhi = icp_cell(px + hx, g.ox, g.inv_c, g.gx);
                            const int rowbase = t * g.gx;
                            s0 = cellStart[rowbase + xlo]; e0 = cellStart[rowbase + xhi + 1];
                            need = e0 > s0;
                        }
                    }
                }
                scan_rows(need, s0, e0);
                if (cnt > kp) { cnt = hyb_rank_cut(sd, si, cnt, kp, nullptr); kth = sd[kp - 1]; }
            }
        }
        cnt = hyb_rank_cut(sd, si, cnt, kp, nullptr);                  // ascending in sd[0 .. k')
        if (lane == 0) {
            double s = 0.0;
            for (int t = 0; t < cnt; ++t) s += sqrt(sd[t]);
            mean_s[jq] = s / (double)kp;
        }
        __syncthreads();
    }
}

// part[block] = sum over the block's elements with mean > 0 of mean (pass 0) or (mean - cloud_mean)^2 (pass 1); the thread's
// elements in index order, the block's 256 sums by a fixed tree
__global__ __launch_bounds__(256) void k_clean_moment(int64_t n, const double* __restrict__ mean_s, const double* __restrict__ stats, int pass,
                                                      double* __restrict__ part) {
    __shared__ double s_a[256];
    const double mu = pass ? stats[0] : 0.0;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double m = mean_s[i];
        if (m > 0.0) acc += pass ? (m - mu) * (m - mu) : m;
    }
    s_a[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_a[threadIdx.x] += s_a[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s_a[0];
}
// stats: cloud_mean, std_dev, threshold.  The partials in block order.
__global__ void k_clean_moment_final(int nb, const double* __restrict__ part, const unsigned long long* __restrict__ ctr, int pass, double std_ratio,
                                     double* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[b];
    const double valid = (double)ctr[CLEAN_CTR_ALIVE];
    if (pass == 0) stats[0] = s / valid;
    else {
        stats[1] = sqrt(s / (valid - 1.0));
        stats[2] = stats[0] + std_ratio * stats[1];
    }
}

__global__ __launch_bounds__(256) void k_clean_stat(int64_t nt, float4* __restrict__ Tq, const double* __restrict__ mean_s, const double* __restrict__ stats,
                                                    uint8_t* __restrict__ stage, double* __restrict__ mean_out) {
    const double thr = stats[2];
    const float nanv = __int_as_float(0x7fc00000);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nt; j += (int64_t)gridDim.x * blockDim.x) {
        const double m = mean_s[j];
        if (!(m >= 0.0)) continue;                                      // did not reach this stage
        const float4 q = Tq[j];
        const int64_t row = (int64_t)__float_as_uint(q.w);
        if (mean_out) mean_out[row] = m;
        if (!(m > 0.0 && m < thr)) {
            stage[row] = CLEAN_STATISTICAL;
            Tq[j] = make_float4(nanv, nanv, nanv, q.w);
        }
    }
}

__global__ __launch_bounds__(256) void k_radius_count(int64_t nt, IcpGrid g, const int* __restrict__ cellStart, const float4* __restrict__ Tq, double r2, int R,
                                                      int nb_points, uint8_t* __restrict__ stage, int* __restrict__ count_out) {
    for (int64_t jq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; jq < nt; jq += (int64_t)gridDim.x * blockDim.x) {
        const float4 qv = Tq[jq];
        const double px = (double)qv.x, py = (double)qv.y, pz = (double)qv.z;
        if (!(px == px && py == py && pz == pz)) continue;
        int count = 0;
        grid_box_walk(g, cellStart, icp_cell(px, g.ox, g.inv_c, g.gx), icp_cell(py, g.oy, g.inv_c, g.gy), icp_cell(pz, g.oz, g.inv_c, g.gz), R, [&](int s0, int e0) {
            for (int j = s0; j < e0; ++j) {
                const float4 q = Tq[j];
                const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
                const double d2 = dx * dx + dy * dy + dz * dz;
                count += d2 < r2 ? 1 : 0;
            }
        });
        const int64_t row = (int64_t)__float_as_uint(qv.w);
        if (count_out) count_out[row] = count;
        if (!(count > nb_points)) stage[row] = CLEAN_RADIUS;
    }
}

__global__ __launch_bounds__(256) void k_clean_mask(int64_t n, const uint8_t* __restrict__ stage, uint8_t* __restrict__ mask, unsigned long long* __restrict__ ctr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = stage[i];
        mask[i] = s == 0 ? 1 : 0;
        wave_count(s == CLEAN_STATISTICAL, ctr + CLEAN_STATISTICAL - 1);
        wave_count(s == CLEAN_RADIUS, ctr + CLEAN_RADIUS - 1);
        wave_count(s == 0, ctr + CLEAN_CTR_KEPT);
    }
}

// ---- row selection
__global__ __launch_bounds__(256) void k_select_flags(int64_t n, const uint8_t* __restrict__ mask, int* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) flag[i] = i < n && mask[i] ? 1 : 0;
}
// sel[scan[i]] = i for the kept rows; the caller's index list takes as many as it holds (cap)
__global__ __launch_bounds__(256) void k_select_index(int64_t n, const uint8_t* __restrict__ mask, const int* __restrict__ scan, int64_t cap,
                                                      int* __restrict__ sel, int* __restrict__ index) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (mask[i]) {
            const int o = scan[i];
            sel[o] = (int)i;
            if (index && o < cap) index[o] = (int)i;
        }
}
// One array of the output, a lane per float (consecutive lanes on consecutive addresses of a row), copied as 32-bit words.
// *total = the number of kept rows; nothing is written behind `cap` rows.
__global__ __launch_bounds__(256) void k_model_select(const int* __restrict__ total, int64_t cap, int W, const int* __restrict__ sel,
                                                      const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const int64_t rows = *total < cap ? *total : cap, words = rows * W;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = t / W;
        const int j = (int)(t - o * W);
        out[t] = in[(int64_t)sel[o] * W + j];
    }
}

namespace {

struct CleanHost {                       // what the one read-back at the end lands in: declared before the OneShot that waits for it
    unsigned long long ctr[CLEAN_NCTR];
    double stats[3];
};

int32_t outlier_mask_run(OneShot& os, GridIndex& gi, Event* ev, CleanHost* host, const float* xyz, const float* raw_opacity, const float* scaling, int64_t n,
                         const gsr_clean_params* P, uint8_t* mask, double* mean_dist, int32_t* count, gsr_clean_report* report) {
    hipStream_t st = os.st;
    size_t workspace = 0;
    auto ws = [&](size_t bytes, auto** p) { workspace += bytes; return os.scratch(bytes, p); };
    const bool gate_op = P->min_raw_opacity > -1.0 / 0.0, gate_sc = P->max_log_scale < 1.0 / 0.0;
    const bool stat_on = P->nb_neighbors >= 1, radius_on = P->radius > 0.0;
    const size_t un = (size_t)n;
    const float *dxyz = nullptr, *dop = nullptr, *dsc = nullptr;
    uint8_t* dmask = nullptr;
    double* dmean = nullptr;
    int32_t* dcount = nullptr;
    GSR_TRY(os.in(xyz, un * 12, &dxyz));
    if (gate_op) GSR_TRY(os.in(raw_opacity, un * 4, &dop));
    if (gate_sc) GSR_TRY(os.in(scaling, un * 12, &dsc));
    GSR_TRY(os.out(mask, un, &dmask));
    GSR_TRY(os.out(mean_dist, un * 8, &dmean));
    GSR_TRY(os.out(count, un * 4, &dcount));
    if (!os.on_device) workspace += un * 12 + (gate_op ? un * 4 : 0) + (gate_sc ? un * 12 : 0) + un + (mean_dist ? un * 8 : 0) + (count ? un * 4 : 0);
    float* sxyz;
    uint8_t* stage;
    unsigned long long* ctr;
    double *stats, *mean_s, *part;
    int* deferred;
    const int nmb = (int)((n + 255) / 256 < CLEAN_MOM_BLOCKS ? (n + 255) / 256 : CLEAN_MOM_BLOCKS);
    GSR_TRY(ws(un * 12 + 8, &sxyz)); GSR_TRY(ws(un + 8, &stage)); GSR_TRY(ws(CLEAN_NCTR * 8, &ctr)); GSR_TRY(ws(4 * 8, &stats));
    GSR_TRY(ws(un * 8 + 8, &mean_s)); GSR_TRY(ws((size_t)CLEAN_MOM_BLOCKS * 8, &part)); GSR_TRY(ws(un * 4 + 8, &deferred));
    GSR_HIP(hipMemsetAsync(ctr, 0, CLEAN_NCTR * 8, st));
    GSR_HIP(hipMemsetAsync(stats, 0, 4 * 8, st));

    // ---- pre-pass and grid
    GSR_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_clean_prep, dim3(stride_grid(n)), dim3(256), 0, st, n, dxyz, dop, dsc, P->min_raw_opacity, P->max_log_scale, sxyz, stage, dmean, dcount, ctr);
    if (stat_on || radius_on) GSR_TRY(gi.build(sxyz, n, radius_on ? P->radius : 1e-300, st));
    const GridView gv = gi.view();
    // ---- k-NN means, moments, the statistical verdict
    GSR_HIP(hipEventRecord(ev[1], st));
    if (stat_on) {
        const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
        const int k = P->nb_neighbors;
#define CLEAN_KNN(KMAX) hipLaunchKernelGGL((k_knn_mean<KMAX>), grid, blk, 0, st, n, gv.g, gv.cellStart, (const float4*)gv.Tq, k, (const unsigned long long*)ctr, mean_s, \
                                           deferred, ctr + CLEAN_CTR_DEFERRED)
        if (k <= 8) CLEAN_KNN(8);
        else if (k <= 16) CLEAN_KNN(16);
        else CLEAN_KNN(32);
#undef CLEAN_KNN
        const int ndb = n < 4096 ? (int)n : 4096;                      // waves for the deferred list: its length is read on the device
        hipLaunchKernelGGL(k_knn_mean_deferred, dim3(ndb), dim3(64), 0, st, gv.g, gv.cellStart, (const float4*)gv.Tq, k, (const unsigned long long*)ctr,
                           (const int*)deferred, mean_s);
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(k_clean_moment, dim3(nmb), dim3(256), 0, st, n, (const double*)mean_s, (const double*)stats, pass, part);
            hipLaunchKernelGGL(k_clean_moment_final, dim3(1), dim3(64), 0, st, nmb, (const double*)part, (const unsigned long long*)ctr, pass, P->std_ratio, stats);
        }
        hipLaunchKernelGGL(k_clean_stat, dim3(stride_grid(n)), dim3(256), 0, st, n, gv.Tq, (const double*)mean_s, (const double*)stats, stage, dmean);
    }
    // ---- radius count
    GSR_HIP(hipEventRecord(ev[2], st));
    if (radius_on) {
        hipLaunchKernelGGL(k_radius_count, dim3(stride_grid(n)), dim3(256), 0, st, n, gv.g, gv.cellStart, (const float4*)gv.Tq, P->radius * P->radius,
                           grid_rings_for_radius(gv.g, P->radius), (int)P->nb_points, stage, dcount);
    }
    // ---- mask
    GSR_HIP(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_clean_mask, dim3(stride_grid(n)), dim3(256), 0, st, n, (const uint8_t*)stage, dmask, ctr);
    GSR_HIP(hipEventRecord(ev[4], st));
    GSR_HIP(hipMemcpyAsync(host->ctr, ctr, sizeof(host->ctr), hipMemcpyDeviceToHost, st));
    GSR_HIP(hipMemcpyAsync(host->stats, stats, sizeof(host->stats), hipMemcpyDeviceToHost, st));
    GSR_TRY(os.finish());
    report->n_nonfinite = (int64_t)host->ctr[CLEAN_NONFINITE - 1];
    report->n_gate_opacity = (int64_t)host->ctr[CLEAN_GATE_OPACITY - 1];
    report->n_gate_scale = (int64_t)host->ctr[CLEAN_GATE_SCALE - 1];
    report->n_statistical = (int64_t)host->ctr[CLEAN_STATISTICAL - 1];
    report->n_radius = (int64_t)host->ctr[CLEAN_RADIUS - 1];
    report->n_kept = (int64_t)host->ctr[CLEAN_CTR_KEPT];
    report->deferred_queries = (int64_t)host->ctr[CLEAN_CTR_DEFERRED];
    report->cloud_mean = host->stats[0]; report->std_dev = host->stats[1]; report->threshold = host->stats[2];
    report->workspace_bytes = (int64_t)workspace;
    for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&report->phase_ms[k], ev[k], ev[k + 1]);
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_outlier_mask(const float* xyz, const float* raw_opacity, const float* scaling, int64_t n, const gsr_clean_params* params, uint8_t* mask,
                                    double* mean_dist, int32_t* count, gsr_clean_report* report, int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_outlier_mask";
    char buf[128];
    if (const char* why = clean_check_args(xyz, raw_opacity, scaling, n, params, mask, report, buf, sizeof(buf))) return fail(GSR_E_INVALID, "%s: %s", who, why);
    GSR_TRY(open_device(device, who));
    memset(report, 0, sizeof(*report));
    report->n = n;
    if (n == 0) return GSR_OK;
    Event ev[5];
    for (Event& e : ev) GSR_HIP(e.create());
    CleanHost host;
    GridIndex gi;                                                      // declared before the OneShot: it waits before the grid's buffers are freed
    OneShot os((hipStream_t)stream, on_device != 0, who);
    return outlier_mask_run(os, gi, ev, &host, xyz, raw_opacity, scaling, n, params, mask, mean_dist, count, report);
}

extern "C" int32_t gsr_model_select(const gsr_model_view* in, int32_t K, const uint8_t* mask, gsr_model_view* out, int32_t* index, int64_t* n_out,
                                    int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_model_select";
    size_t width[GSR_MODEL_NARR];
    bool used[GSR_MODEL_NARR];
    if (const char* why = select_check_args(in, K, mask, out, index, n_out, width, used)) return fail(GSR_E_INVALID, "%s: %s", who, why);
    GSR_TRY(open_device(device, who));
    const int64_t n = in->n, cap = out->n;
    *n_out = 0;
    if (n == 0) { out->n = 0; return GSR_OK; }
    const bool dev = on_device != 0;
    const size_t un = (size_t)n, ucap = (size_t)cap;
    DevBuf tmp_scan;                                                   // rocPRIM's temporary: declared before the OneShot, freed after its wait
    int total = 0;
    OneShot os((hipStream_t)stream, dev, who);
    hipStream_t st = os.st;
    const uint8_t* dmask = nullptr;
    GSR_TRY(os.in(mask, un, &dmask));
    const float* din[GSR_MODEL_NARR] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* dout[GSR_MODEL_NARR];
    if (cap > 0) GSR_TRY(model_in(os, in, width, used, din));          // (an output without rows takes none)
    GSR_TRY(model_out(os, out, cap, width, used, dout));
    int32_t* dindex = nullptr;
    if (index && cap > 0) { if (dev) dindex = index; else GSR_TRY(os.scratch(ucap * 4, &dindex)); }
    int *flag, *scan, *sel;
    GSR_TRY(os.scratch((un + 1) * 4, &flag)); GSR_TRY(os.scratch((un + 1) * 4, &scan)); GSR_TRY(os.scratch(un * 4 + 8, &sel));
    hipLaunchKernelGGL(k_select_flags, dim3(stride_grid(n + 1)), dim3(256), 0, st, n, dmask, flag);
    GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan, st, (const int*)flag, scan, un + 1));
    hipLaunchKernelGGL(k_select_index, dim3(stride_grid(n)), dim3(256), 0, st, n, dmask, (const int*)scan, cap, sel, dindex);
    const int64_t rows_max = n < cap ? n : cap;
    for (int k = 0; k < GSR_MODEL_NARR; ++k)
        if (dout[k])
            hipLaunchKernelGGL(k_model_select, dim3(stride_grid(rows_max * (int64_t)width[k])), dim3(256), 0, st, (const int*)scan + n, cap, (int)width[k],
                               (const int*)sel, reinterpret_cast<const uint32_t*>(din[k]), reinterpret_cast<uint32_t*>(dout[k]));
    // ---- the one read-back: the count
    GSR_HIP(hipMemcpyAsync(&total, scan + n, 4, hipMemcpyDeviceToHost, st));
    GSR_TRY(os.wait());
    *n_out = total;
    if (total > cap) return fail(GSR_E_INVALID, "%s: %d rows are kept, the output holds %lld", who, total, (long long)cap);
    GSR_TRY(model_copy_back(os, out, dout, total, width));
    if (!dev && dindex && total > 0) GSR_HIP(hipMemcpyAsync(index, dindex, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    out->n = total;
    return os.finish();
}
