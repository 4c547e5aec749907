// features.hip -- global registration on MI355X (gfx950), behind include/gsr_hip.h: FPFH features, feature matching and RANSAC over
// correspondences, the work of the reference's "Global" tab (src/utils/global_registration_util.py) through Open3D 0.16.
//
//   gsr_hybrid_search   KDTreeSearchParamHybrid(radius, max_nn) of the cloud against itself (k_hybrid_search in grid.hip, on a
//                       point grid of the cloud)
//   gsr_fpfh            k_spfh (thread per point: pair features of its neighbourhood, bin counts in LDS) then k_fpfh (thread per
//                       point: 33 float64 accumulators over the neighbours' SPFH rows)
//   gsr_feature_match   k_fm_nn: exact float64 1-NN over 33 dimensions, a source row per thread in registers against target tiles
//                       staged in LDS, the target split into chunks over blockIdx.y; k_fm_merge takes the chunks in order
//   gsr_ransac_*        k_ransac_hyp (thread per hypothesis: counter-based draw, estimate, checkers) and k_ransac_eval (a block per
//                       RANSAC_HB hypotheses, a correspondence per thread and trip, per-thread float64 sums reduced by a fixed tree);
//                       the host replays Open3D's serial selection rule over each batch
#include "gsr_common.h"
#include "gsr_features.h"
#include "gsr_oneshot.h"
#include "gsr_solve.h"
#include "gsr_test_hooks.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace gsr {

// ---- FPFH --------------------------------------------------------------------------------------------------------------------
// Open3D 0.16 ComputePairFeatures (Feature.cpp): (phi, alpha, theta) of the Darboux frame, in float64.  Returns false, with
// f = (0, 0, 0) written on both paths, for the zero vector: coincident points (len == 0) or p2 - p1 parallel to the frame normal
// (v_norm == 0; theta, stored before that test, is cleared again).
__device__ __forceinline__ bool pair_features(const double p1[3], const double n1[3], const double p2[3], const double n2[3], double f[3]) {
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double len = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
    f[0] = 0.0; f[1] = 0.0; f[2] = 0.0;
    if (len == 0.0) return false;
    double a[3] = {n1[0], n1[1], n1[2]}, b[3] = {n2[0], n2[1], n2[2]};
    const double angle1 = (a[0] * dp[0] + a[1] * dp[1] + a[2] * dp[2]) / len;
    const double angle2 = (b[0] * dp[0] + b[1] * dp[1] + b[2] * dp[2]) / len;
    if (acos(fabs(angle1)) > acos(fabs(angle2))) {
        for (int k = 0; k < 3; ++k) { const double t = a[k]; a[k] = b[k]; b[k] = t; dp[k] = -dp[k]; }
        f[2] = -angle2;
    } else {
        f[2] = angle1;
    }
    double v[3] = {dp[1] * a[2] - dp[2] * a[1], dp[2] * a[0] - dp[0] * a[2], dp[0] * a[1] - dp[1] * a[0]};
    const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (vn == 0.0) { f[2] = 0.0; return false; }
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    const double w[3] = {a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]};
    f[1] = v[0] * b[0] + v[1] * b[1] + v[2] * b[2];
    f[0] = atan2(w[0] * b[0] + w[1] * b[1] + w[2] * b[2], a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
    return true;
}

__device__ __forceinline__ int fpfh_bin(double v) {
    int h = (int)floor(v);
    return h < 0 ? 0 : (h >= 11 ? 10 : h);
}

#define SPFH_BLOCK 128
// SPFH of every point: bin counts of its pair features with neighbours 1 .. k-1 (entry 0 of the sorted list is skipped, as Open3D
// does), times 100 / (k - 1).  (Open3D adds the increment once per pair; count * increment differs from that sum by < 1e-12.)
__global__ __launch_bounds__(SPFH_BLOCK) void k_spfh(int64_t n, const float* __restrict__ xyz, const double* __restrict__ nrm,
                                                     const int* __restrict__ nbr, const int* __restrict__ cnt, int max_nn,
                                                     double* __restrict__ spfh) {
    __shared__ unsigned hist[33 * SPFH_BLOCK];
    const int t = threadIdx.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + t; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        for (int b = 0; b < 33; ++b) hist[b * SPFH_BLOCK + t] = 0u;
        const int k = cnt[i];
        const double p1[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        const double n1[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
        for (int e = 1; e < k; ++e) {
            const int64_t j = nbr[i * max_nn + e];
            const double p2[3] = {(double)xyz[3 * j], (double)xyz[3 * j + 1], (double)xyz[3 * j + 2]};
            const double n2[3] = {nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]};
            double f[3] = {0.0, 0.0, 0.0};
            (void)pair_features(p1, n1, p2, n2, f);                       // the zero vector still counts (bins 5 / 5 / 5)
            hist[fpfh_bin(11.0 * (f[0] + M_PI) / (2.0 * M_PI)) * SPFH_BLOCK + t] += 1u;
            hist[(11 + fpfh_bin(11.0 * (f[1] + 1.0) * 0.5)) * SPFH_BLOCK + t] += 1u;
            hist[(22 + fpfh_bin(11.0 * (f[2] + 1.0) * 0.5)) * SPFH_BLOCK + t] += 1u;
        }
        const double incr = k > 1 ? 100.0 / (double)(k - 1) : 0.0;
        for (int b = 0; b < 33; ++b) spfh[33 * i + b] = k > 1 ? (double)hist[b * SPFH_BLOCK + t] * incr : 0.0;
    }
}

// FPFH of every point: sum over neighbours 1 .. k-1 of SPFH[j] / d2 (d2 == 0 skipped), each third scaled to 100, plus SPFH[i].
__global__ __launch_bounds__(256) void k_fpfh(int64_t n, const float* __restrict__ xyz, const int* __restrict__ nbr, const int* __restrict__ cnt,
                                              int max_nn, const double* __restrict__ spfh, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = cnt[i];
        double acc[33];
#pragma unroll
        for (int b = 0; b < 33; ++b) acc[b] = 0.0;
        if (k > 1) {
            double sum[3] = {0.0, 0.0, 0.0};
            const double px = (double)xyz[3 * i], py = (double)xyz[3 * i + 1], pz = (double)xyz[3 * i + 2];
            for (int e = 1; e < k; ++e) {
                const int64_t j = nbr[i * max_nn + e];
                const double dx = px - (double)xyz[3 * j], dy = py - (double)xyz[3 * j + 1], dz = pz - (double)xyz[3 * j + 2];
                const double d2 = dx * dx + dy * dy + dz * dz;           // the search's d2, bit for bit
                if (d2 == 0.0) continue;
                const double* s = spfh + 33 * j;
#pragma unroll
                for (int b = 0; b < 33; ++b) {
                    const double v = s[b] / d2;
                    sum[b / 11] += v;
                    acc[b] += v;
                }
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) if (sum[q] != 0.0) sum[q] = 100.0 / sum[q];
#pragma unroll
            for (int b = 0; b < 33; ++b) acc[b] = acc[b] * sum[b / 11] + spfh[33 * i + b];
        }
#pragma unroll
        for (int b = 0; b < 33; ++b) out[33 * i + b] = acc[b];
    }
}

// ---- feature matching ----------------------------------------------------------------------------------------------------------
#define FM_BLOCK 256
#define FM_TILE 32
// best[c * na + i] / bestd: the nearest row of b[lo .. hi) (chunk c = blockIdx.y) to a[i], ties to the lowest index.  Distances
// are sum_j (a_j - b_j)^2 in j order; this file is compiled with -ffp-contract=off, so each step rounds as written.
__global__ __launch_bounds__(FM_BLOCK) void k_fm_nn(int64_t na, const double* __restrict__ a, int64_t nb, const double* __restrict__ b,
                                                    int64_t chunk, int* __restrict__ best, double* __restrict__ bestd) {
    __shared__ double tile[FM_TILE * 33];
    const int64_t i = (int64_t)blockIdx.x * FM_BLOCK + threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.y * chunk, hi = lo + chunk < nb ? lo + chunk : nb;
    double q[33];
#pragma unroll
    for (int d = 0; d < 33; ++d) q[d] = i < na ? a[33 * i + d] : 0.0;
    double bd = 1.0 / 0.0;
    int bi = -1;
    for (int64_t t0 = lo; t0 < hi; t0 += FM_TILE) {
        const int rows = hi - t0 < FM_TILE ? (int)(hi - t0) : FM_TILE;
        __syncthreads();
        for (int e = threadIdx.x; e < rows * 33; e += FM_BLOCK) tile[e] = b[33 * t0 + e];
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            double d = 0.0;
#pragma unroll
            for (int k = 0; k < 33; ++k) {
                const double df = q[k] - tile[33 * r + k];
                d += df * df;
            }
            if (d < bd) { bd = d; bi = (int)(t0 + r); }
        }
    }
    if (i < na) { best[blockIdx.y * na + i] = bi; bestd[blockIdx.y * na + i] = bd; }
}

__global__ __launch_bounds__(256) void k_fm_merge(int64_t na, int nchunks, const int* __restrict__ best, const double* __restrict__ bestd,
                                                  int* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < na; i += (int64_t)gridDim.x * blockDim.x) {
        double bd = 1.0 / 0.0;
        int bi = -1;
        for (int c = 0; c < nchunks; ++c) {
            const double d = bestd[c * na + i];
            const int j = best[c * na + i];
            if (j >= 0 && (bi < 0 || d < bd)) { bd = d; bi = j; }
        }
        out[i] = bi < 0 ? 0 : bi;             // (a row of NaN features: Open3D's KD-tree gives some row; here row 0)
    }
}

namespace {
// nearest rows of b for every row of a (device arrays), into out[na] (device)
int32_t nn_rows(OneShot& os, const double* a, int64_t na, const double* b, int64_t nb, int* out) {
    if (na <= 0) return GSR_OK;
    const int64_t gx = (na + FM_BLOCK - 1) / FM_BLOCK;
    // enough workgroups to fill the chip twice over (256 CUs), each chunk at least 512 target rows
    int64_t nch = (2048 + gx - 1) / gx;
    const int64_t maxch = (nb + 511) / 512;
    if (nch > maxch) nch = maxch;
    if (nch < 1) nch = 1;
    if (nch > 65535) nch = 65535;
    const int64_t chunk = (nb + nch - 1) / nch;
    nch = (nb + chunk - 1) / chunk;
    int* wi = nullptr;
    double* wd = nullptr;
    GSR_TRY(os.scratch((size_t)(nch * na) * 4, &wi));
    GSR_TRY(os.scratch((size_t)(nch * na) * 8, &wd));
    hipLaunchKernelGGL(k_fm_nn, dim3((unsigned)gx, (unsigned)nch), dim3(FM_BLOCK), 0, os.st, na, a, nb, b, chunk, wi, wd);
    hipLaunchKernelGGL(k_fm_merge, dim3(stride_grid(na)), dim3(256), 0, os.st, na, (int)nch, wi, wd, out);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}
}  // namespace

// ---- RANSAC ------------------------------------------------------------------------------------------------------------------
// splitmix64 / ransac_draw: gsr_features.h (csrc/fgr.hip draws its triples with the same function)
struct RansacDev {
    int kind, n, n_checkers, has_normals;
    int ck[4];
    double cp[4];
    double mc2;
    uint64_t seed;
    int64_t m;
};

// Hypothesis k0 + t: draw, sort, estimate, check.  T[12 * t] = rows 0..2 of the 4x4, valid[t] = 1 if it goes on to the evaluation.
// P / Q: the correspondences' source / target points (float64), NS / NT their normals (NULL if absent).
__global__ __launch_bounds__(64) void k_ransac_hyp(int64_t k0, int nb, RansacDev a, const double* __restrict__ P, const double* __restrict__ Q,
                                                   const double* __restrict__ NS, const double* __restrict__ NT, double* __restrict__ Tout,
                                                   int* __restrict__ valid) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb) return;
    const int n = a.n;
    uint32_t idx[GSR_RANSAC_MAX_N];
    for (int j = 0; j < n; ++j) idx[j] = ransac_draw(a.seed, (uint64_t)(k0 + t), (uint32_t)j, (uint32_t)a.m);
    for (int j = 1; j < n; ++j) {                    // insertion sort: the hypothesis is a set
        const uint32_t v = idx[j];
        int p = j;
        while (p > 0 && idx[p - 1] > v) { idx[p] = idx[p - 1]; --p; }
        idx[p] = v;
    }
    bool ok = true;
    for (int j = 1; j < n; ++j) ok = ok && idx[j] != idx[j - 1];
    double update[16];
    mat4_identity(update);
    if (ok) {
        double acc[GSR_ICP_ACC_LEN];
        for (int e = 0; e < GSR_ICP_ACC_LEN; ++e) acc[e] = 0.0;
        acc[0] = (double)n;
        for (int j = 0; j < n; ++j) {
            const int64_t c = idx[j];
            const double p[3] = {P[3 * c], P[3 * c + 1], P[3 * c + 2]}, q[3] = {Q[3 * c], Q[3 * c + 1], Q[3 * c + 2]};
            if (a.kind == GSR_ICP_POINT_TO_POINT || a.kind == GSR_ICP_POINT_TO_POINT_SCALED) {
                for (int r = 0; r < 3; ++r) { acc[2 + r] += p[r]; acc[5 + r] += q[r]; }
                for (int r = 0; r < 3; ++r) for (int s = 0; s < 3; ++s) acc[8 + 3 * r + s] += p[r] * q[s];
                if (a.kind == GSR_ICP_POINT_TO_POINT_SCALED) acc[17] += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
            } else {
                const double nt[3] = {NT[3 * c], NT[3 * c + 1], NT[3 * c + 2]};
                const double rr = (p[0] - q[0]) * nt[0] + (p[1] - q[1]) * nt[1] + (p[2] - q[2]) * nt[2];
                const double J[6] = {p[1] * nt[2] - p[2] * nt[1], p[2] * nt[0] - p[0] * nt[2], p[0] * nt[1] - p[1] * nt[0], nt[0], nt[1], nt[2]};
                int e = 2;
                for (int r = 0; r < 6; ++r) for (int s = r; s < 6; ++s) acc[e++] += J[r] * J[s];
                for (int r = 0; r < 6; ++r) acc[23 + r] += J[r] * rr;
            }
        }
        const double zero[3] = {0.0, 0.0, 0.0};
        estimate_update(zero, a.kind, acc, update);
        for (int e = 0; e < 12; ++e) ok = ok && isfinite(update[e]);     // a singular system (point-to-plane on fewer than 6 rows)
        for (int ci = 0; ci < a.n_checkers && ok; ++ci) {
            const double thr = a.cp[ci];
            if (a.ck[ci] == GSR_CHECK_EDGE_LENGTH) {
                for (int i = 0; i < n && ok; ++i)
                    for (int j = i + 1; j < n && ok; ++j) {
                        const int64_t ci_ = idx[i], cj = idx[j];
                        const double sx = P[3 * ci_] - P[3 * cj], sy = P[3 * ci_ + 1] - P[3 * cj + 1], sz = P[3 * ci_ + 2] - P[3 * cj + 2];
                        const double tx = Q[3 * ci_] - Q[3 * cj], ty = Q[3 * ci_ + 1] - Q[3 * cj + 1], tz = Q[3 * ci_ + 2] - Q[3 * cj + 2];
                        const double ds = sqrt(sx * sx + sy * sy + sz * sz), dt = sqrt(tx * tx + ty * ty + tz * tz);
                        if (ds < dt * thr || dt < ds * thr) ok = false;
                    }
            } else if (a.ck[ci] == GSR_CHECK_DISTANCE) {
                for (int j = 0; j < n && ok; ++j) {
                    const int64_t c = idx[j];
                    double d2 = 0.0;
                    for (int r = 0; r < 3; ++r) {
                        const double x = update[4 * r] * P[3 * c] + update[4 * r + 1] * P[3 * c + 1] + update[4 * r + 2] * P[3 * c + 2] + update[4 * r + 3];
                        const double df = Q[3 * c + r] - x;
                        d2 += df * df;
                    }
                    if (sqrt(d2) > thr) ok = false;
                }
            } else if (a.ck[ci] == GSR_CHECK_NORMAL && a.has_normals) {
                const double cth = cos(thr);
                // a scaled hypothesis is A = c R: normals turn by R = A / c (c = cbrt(det A) > 0 by construction)
                double ic = 1.0;
                if (a.kind == GSR_ICP_POINT_TO_POINT_SCALED) {
                    const double A3[3][3] = {{update[0], update[1], update[2]}, {update[4], update[5], update[6]}, {update[8], update[9], update[10]}};
                    ic = 1.0 / cbrt(det3(A3));
                }
                for (int j = 0; j < n && ok; ++j) {
                    const int64_t c = idx[j];
                    double dot = 0.0;
                    for (int r = 0; r < 3; ++r)
                        dot += NT[3 * c + r] * (update[4 * r] * NS[3 * c] + update[4 * r + 1] * NS[3 * c + 1] + update[4 * r + 2] * NS[3 * c + 2]);
                    if (dot * ic < cth) ok = false;
                }
            }
        }
    }
    for (int e = 0; e < 12; ++e) Tout[12 * (int64_t)t + e] = update[e];
    valid[t] = ok ? 1 : 0;
}

#define RANSAC_HB 4
#define RANSAC_EVAL_BLOCK 256
// Inlier count and sum of d2 of RANSAC_HB hypotheses per block over all m correspondences: thread t takes the correspondences
// t, t + 256, ... in ascending order (its sum starts at 0), then a fixed tree over the 256 partial sums (stride 128, 64, ..., 1).
// The order depends on neither the batch size nor the hypothesis' slot.  No atomics.
__global__ __launch_bounds__(RANSAC_EVAL_BLOCK) void k_ransac_eval(int nb, int64_t m, double mc2, const double* __restrict__ P,
                                                                   const double* __restrict__ Q, const double* __restrict__ T,
                                                                   const int* __restrict__ valid, double* __restrict__ fit,
                                                                   double* __restrict__ rmse) {
    __shared__ double s_sum[RANSAC_EVAL_BLOCK];
    __shared__ unsigned s_cnt[RANSAC_EVAL_BLOCK];
    const int tid = threadIdx.x;
    const int h0 = blockIdx.x * RANSAC_HB;
    double M[RANSAC_HB][12];
#pragma unroll
    for (int h = 0; h < RANSAC_HB; ++h)
#pragma unroll
        for (int e = 0; e < 12; ++e) M[h][e] = h0 + h < nb ? T[12 * (int64_t)(h0 + h) + e] : 0.0;
    double sum[RANSAC_HB];
    unsigned cnt[RANSAC_HB];
    bool live[RANSAC_HB];           // a hypothesis k_ransac_hyp rejected is not evaluated (its sums stay 0; it reports -1 anyway)
#pragma unroll
    for (int h = 0; h < RANSAC_HB; ++h) { sum[h] = 0.0; cnt[h] = 0u; live[h] = h0 + h < nb && valid[h0 + h] != 0; }
    bool any = false;
#pragma unroll
    for (int h = 0; h < RANSAC_HB; ++h) any = any || live[h];
    const int64_t m_eval = any ? m : 0;
    for (int64_t c = tid; c < m_eval; c += RANSAC_EVAL_BLOCK) {
        const double px = P[3 * c], py = P[3 * c + 1], pz = P[3 * c + 2];
        const double qx = Q[3 * c], qy = Q[3 * c + 1], qz = Q[3 * c + 2];
#pragma unroll
        for (int h = 0; h < RANSAC_HB; ++h) {
            const double x = M[h][0] * px + M[h][1] * py + M[h][2] * pz + M[h][3];
            const double y = M[h][4] * px + M[h][5] * py + M[h][6] * pz + M[h][7];
            const double z = M[h][8] * px + M[h][9] * py + M[h][10] * pz + M[h][11];
            const double dx = x - qx, dy = y - qy, dz = z - qz;
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (live[h] && d2 < mc2) { sum[h] += d2; cnt[h] += 1u; }
        }
    }
#pragma unroll
    for (int h = 0; h < RANSAC_HB; ++h) {
        __syncthreads();
        s_sum[tid] = sum[h]; s_cnt[tid] = cnt[h];
        __syncthreads();
        for (int s = RANSAC_EVAL_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) { s_sum[tid] += s_sum[tid + s]; s_cnt[tid] += s_cnt[tid + s]; }
            __syncthreads();
        }
        if (tid == 0 && h0 + h < nb) {
            const unsigned g = s_cnt[0];
            const bool ok = valid[h0 + h] != 0;
            fit[h0 + h] = ok ? (double)g / (double)m : -1.0;
            rmse[h0 + h] = ok && g > 0 ? sqrt(s_sum[0] / (double)g) : 0.0;
        }
    }
}

// P / Q (and normals) of the correspondences, float64
__global__ __launch_bounds__(256) void k_ransac_gather(int64_t m, const int* __restrict__ corres, const float* __restrict__ sx, const float* __restrict__ tx,
                                                       const double* __restrict__ sn, const double* __restrict__ tn, double* __restrict__ P,
                                                       double* __restrict__ Q, double* __restrict__ NS, double* __restrict__ NT) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < m; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = corres[2 * c], j = corres[2 * c + 1];
        for (int r = 0; r < 3; ++r) {
            P[3 * c + r] = (double)sx[3 * i + r];
            Q[3 * c + r] = (double)tx[3 * j + r];
            if (NS) NS[3 * c + r] = sn[3 * i + r];
            if (NT) NT[3 * c + r] = tn[3 * j + r];
        }
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_hybrid_search(const float* xyz, int64_t n, double radius, int32_t max_nn, int32_t* nbr, int32_t* count, int32_t on_device,
                          int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!xyz || !nbr || !count))) return fail(GSR_E_INVALID, "gsr_hybrid_search: bad argument");
    if (max_nn < 1 || max_nn > GSR_HYBRID_MAX_NN) return fail(GSR_E_INVALID, "gsr_hybrid_search: max_nn must lie in [1, %d] (got %d)", GSR_HYBRID_MAX_NN, max_nn);
    if (!(radius > 0.0)) return fail(GSR_E_INVALID, "gsr_hybrid_search: radius must be > 0");
    if (n == 0) return GSR_OK;
    GSR_TRY(open_device(device, "gsr_hybrid_search"));
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_hybrid_search");
    const float* dxyz = nullptr;
    int *dnbr = nullptr, *dcnt = nullptr;
    GSR_TRY(os.in(xyz, (size_t)n * 12, &dxyz));
    GSR_TRY(os.out(nbr, (size_t)n * max_nn * 4, &dnbr));
    GSR_TRY(os.out(count, (size_t)n * 4, &dcnt));
    GSR_TRY(hybrid_search_dev(dxyz, n, radius, max_nn, device, os.st, dnbr, dcnt));
    return os.finish();
}

int32_t gsr_fpfh(const float* xyz, const double* normals, int64_t n, double radius, int32_t max_nn, double* out, int32_t on_device,
                 int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!xyz || !normals || !out))) return fail(GSR_E_INVALID, "gsr_fpfh: bad argument (xyz, normals and out are required)");
    if (max_nn < 1 || max_nn > GSR_HYBRID_MAX_NN) return fail(GSR_E_INVALID, "gsr_fpfh: max_nn must lie in [1, %d] (got %d)", GSR_HYBRID_MAX_NN, max_nn);
    if (!(radius > 0.0)) return fail(GSR_E_INVALID, "gsr_fpfh: radius must be > 0");
    if (n == 0) return GSR_OK;
    GSR_TRY(open_device(device, "gsr_fpfh"));
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_fpfh");
    const float* dxyz = nullptr;
    const double* dnrm = nullptr;
    int *nbr = nullptr, *cnt = nullptr;
    double *spfh = nullptr, *o = nullptr;
    GSR_TRY(os.in(xyz, (size_t)n * 12, &dxyz));
    GSR_TRY(os.in(normals, (size_t)n * 24, &dnrm));
    GSR_TRY(os.scratch((size_t)n * max_nn * 4, &nbr));
    GSR_TRY(os.scratch((size_t)n * 4, &cnt));
    GSR_TRY(os.scratch((size_t)n * 33 * 8, &spfh));
    GSR_TRY(os.out(out, (size_t)n * 33 * 8, &o));
    GSR_TRY(hybrid_search_dev(dxyz, n, radius, max_nn, device, os.st, nbr, cnt));
    hipLaunchKernelGGL(k_spfh, dim3(ceil_div(n, SPFH_BLOCK) < 4096 ? ceil_div(n, SPFH_BLOCK) : 4096), dim3(SPFH_BLOCK), 0, os.st, n, dxyz, dnrm, nbr, cnt,
                       max_nn, spfh);
    hipLaunchKernelGGL(k_fpfh, dim3(stride_grid(n)), dim3(256), 0, os.st, n, dxyz, nbr, cnt, max_nn, spfh, o);
    return os.finish();
}

int32_t gsr_feature_match(const double* src_feat, int64_t ns, const double* tgt_feat, int64_t nt, int32_t mutual, int32_t ransac_n,
                          int32_t* corres, int64_t* n_corres, int32_t* used_mutual, int32_t* nn_st, int32_t* nn_ts, int32_t on_device,
                          int32_t device, void* stream) {
    if (ns < 0 || nt < 0 || !n_corres || (ns > 0 && (!src_feat || !corres)) || (nt > 0 && !tgt_feat))
        return fail(GSR_E_INVALID, "gsr_feature_match: bad argument");
    *n_corres = 0;
    if (used_mutual) *used_mutual = 0;
    if (ns == 0) return GSR_OK;
    if (nt == 0) return fail(GSR_E_INVALID, "gsr_feature_match: empty target feature set");
    if (ns >= ((int64_t)1 << 31) || nt >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "gsr_feature_match: more than 2^31 rows");
    GSR_TRY(open_device(device, "gsr_feature_match"));
    std::vector<int32_t> h_st((size_t)ns), h_ts(mutual ? (size_t)nt : 0), pairs;      // before `os`: it waits for the copies into them
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_feature_match");
    const double *da = nullptr, *db = nullptr;
    int *dst = nullptr, *dts = nullptr;
    GSR_TRY(os.in(src_feat, (size_t)ns * 33 * 8, &da));
    GSR_TRY(os.in(tgt_feat, (size_t)nt * 33 * 8, &db));
    GSR_TRY(os.scratch((size_t)ns * 4, &dst));
    if (mutual) GSR_TRY(os.scratch((size_t)nt * 4, &dts));
    GSR_TRY(nn_rows(os, da, ns, db, nt, dst));
    if (mutual) GSR_TRY(nn_rows(os, db, nt, da, ns, dts));
    GSR_HIP(hipMemcpyAsync(h_st.data(), dst, (size_t)ns * 4, hipMemcpyDeviceToHost, os.st));
    if (mutual) GSR_HIP(hipMemcpyAsync(h_ts.data(), dts, (size_t)nt * 4, hipMemcpyDeviceToHost, os.st));
    GSR_TRY(os.wait());
    // the pair list is O(n) host work on the read-back indices
    pairs.reserve((size_t)ns * 2);
    bool use_mutual = false;
    if (mutual) {
        for (int64_t i = 0; i < ns; ++i)
            if (h_ts[h_st[i]] == (int32_t)i) { pairs.push_back((int32_t)i); pairs.push_back(h_st[i]); }
        use_mutual = (int64_t)(pairs.size() / 2) >= 3 * (int64_t)ransac_n;
    }
    if (!use_mutual) {
        pairs.clear();
        for (int64_t i = 0; i < ns; ++i) { pairs.push_back((int32_t)i); pairs.push_back(h_st[i]); }
    }
    *n_corres = (int64_t)(pairs.size() / 2);
    if (used_mutual) *used_mutual = use_mutual ? 1 : 0;
    const hipMemcpyKind dk = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (on_device) GSR_HIP(hipMemcpyAsync(corres, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, os.st));
    else memcpy(corres, pairs.data(), pairs.size() * 4);
    if (nn_st) GSR_HIP(hipMemcpyAsync(nn_st, dst, (size_t)ns * 4, dk, os.st));
    if (nn_ts && mutual) GSR_HIP(hipMemcpyAsync(nn_ts, dts, (size_t)nt * 4, dk, os.st));
    return os.finish();
}

int32_t gsr_ransac_correspondence(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const double* src_normals,
                                  const double* tgt_normals, const int32_t* corres, int64_t m, const gsr_ransac_params* params,
                                  gsr_ransac_result* out, int32_t on_device, int32_t device, void* stream) {
    if (!params || !out || ns < 0 || nt < 0 || m < 0) return fail(GSR_E_INVALID, "gsr_ransac_correspondence: bad argument");
    const gsr_ransac_params& P = *params;
    memset(out, 0, sizeof(*out));
    mat4_identity(out->T);
    out->best_index = -1;
    if (P.kind != GSR_ICP_POINT_TO_POINT && P.kind != GSR_ICP_POINT_TO_PLANE && P.kind != GSR_ICP_POINT_TO_POINT_SCALED)
        return fail(GSR_E_INVALID, "gsr_ransac_correspondence: estimation kind %d is not supported (point-to-point, plain or scaled, or point-to-plane)", P.kind);
    if (P.n_checkers < 0 || P.n_checkers > 4) return fail(GSR_E_INVALID, "gsr_ransac_correspondence: at most 4 checkers");
    for (int c = 0; c < P.n_checkers; ++c)
        if (P.checker_kind[c] < GSR_CHECK_EDGE_LENGTH || P.checker_kind[c] > GSR_CHECK_NORMAL)
            return fail(GSR_E_INVALID, "gsr_ransac_correspondence: unknown checker %d", P.checker_kind[c]);
    if (P.ransac_n > GSR_RANSAC_MAX_N) return fail(GSR_E_INVALID, "gsr_ransac_correspondence: ransac_n must be <= %d", GSR_RANSAC_MAX_N);
    // Open3D's empty result
    if (P.ransac_n < 3 || m < P.ransac_n || !(P.max_corr > 0.0) || P.max_iteration <= 0) return GSR_OK;
    if (!src_xyz || !tgt_xyz || !corres) return fail(GSR_E_INVALID, "gsr_ransac_correspondence: NULL cloud or correspondences");
    if (P.kind == GSR_ICP_POINT_TO_PLANE && !tgt_normals)
        return fail(GSR_E_PRECONDITION, "gsr_ransac_correspondence: point-to-plane needs target normals");
    if (m >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "gsr_ransac_correspondence: too many correspondences");
    if (!on_device) {       // bounds of the rows (device arrays are the caller's responsibility, as everywhere in this ABI)
        for (int64_t c = 0; c < m; ++c)
            if (corres[2 * c] < 0 || corres[2 * c] >= ns || corres[2 * c + 1] < 0 || corres[2 * c + 1] >= nt)
                return fail(GSR_E_INVALID, "gsr_ransac_correspondence: correspondence %lld out of range", (long long)c);
    }
    GSR_TRY(open_device(device, "gsr_ransac_correspondence"));
    const bool has_normals = src_normals && tgt_normals;
    int B = P.batch > 0 ? P.batch : 8192;
    if (B > (1 << 20)) B = 1 << 20;
    std::vector<double> hfit((size_t)B), hrmse((size_t)B);       // before `os`: it waits for the copies into them
    double best_T[12];                                           // *out keeps the empty result until the call has succeeded
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_ransac_correspondence");
    const float *sx = nullptr, *tx = nullptr;
    const double *sn = nullptr, *tn = nullptr;
    const int32_t* dc = nullptr;
    double *dP = nullptr, *dQ = nullptr, *dNS = nullptr, *dNT = nullptr, *dT = nullptr, *dfit = nullptr, *drmse = nullptr;
    int* dvalid = nullptr;
    GSR_TRY(os.in(src_xyz, (size_t)ns * 12, &sx));
    GSR_TRY(os.in(tgt_xyz, (size_t)nt * 12, &tx));
    if (has_normals) GSR_TRY(os.in(src_normals, (size_t)ns * 24, &sn));
    GSR_TRY(os.in(tgt_normals, (size_t)nt * 24, &tn));
    GSR_TRY(os.in(corres, (size_t)m * 8, &dc));
    GSR_TRY(os.scratch((size_t)m * 24, &dP));
    GSR_TRY(os.scratch((size_t)m * 24, &dQ));
    if (has_normals) GSR_TRY(os.scratch((size_t)m * 24, &dNS));
    if (tn) GSR_TRY(os.scratch((size_t)m * 24, &dNT));
    GSR_TRY(os.scratch((size_t)B * 96, &dT));
    GSR_TRY(os.scratch((size_t)B * 4, &dvalid));
    GSR_TRY(os.scratch((size_t)B * 8, &dfit));
    GSR_TRY(os.scratch((size_t)B * 8, &drmse));
    hipLaunchKernelGGL(k_ransac_gather, dim3(stride_grid(m)), dim3(256), 0, os.st, m, (const int*)dc, sx, tx, sn, tn, dP, dQ, dNS, dNT);
    RansacDev a;
    a.kind = P.kind; a.n = P.ransac_n; a.n_checkers = P.n_checkers; a.has_normals = has_normals ? 1 : 0;
    for (int c = 0; c < 4; ++c) { a.ck[c] = c < P.n_checkers ? P.checker_kind[c] : -1; a.cp[c] = c < P.n_checkers ? P.checker_param[c] : 0.0; }
    a.mc2 = P.max_corr * P.max_corr; a.seed = P.seed; a.m = m;
    int64_t exit_k = P.max_iteration, k = 0, best = -1, n_valid = 0;
    double best_fit = 0.0, best_rmse = 0.0;
    while (k < exit_k) {
        const int nb = (int)std::min<int64_t>(B, P.max_iteration - k);
        hipLaunchKernelGGL(k_ransac_hyp, dim3((nb + 63) / 64), dim3(64), 0, os.st, k, nb, a, dP, dQ, dNS, dNT, dT, dvalid);
        hipLaunchKernelGGL(k_ransac_eval, dim3((nb + RANSAC_HB - 1) / RANSAC_HB), dim3(RANSAC_EVAL_BLOCK), 0, os.st, nb, m, a.mc2, dP, dQ, dT, dvalid,
                           dfit, drmse);
        GSR_HIP(hipMemcpyAsync(hfit.data(), dfit, (size_t)nb * 8, hipMemcpyDeviceToHost, os.st));
        GSR_HIP(hipMemcpyAsync(hrmse.data(), drmse, (size_t)nb * 8, hipMemcpyDeviceToHost, os.st));
        GSR_TRY(os.wait());
        int64_t best_in_batch = -1;
        // Open3D's serial rule, hypothesis by hypothesis in index order
        for (int t = 0; t < nb && k < exit_k; ++t, ++k) {
            const double f = hfit[t], rm = hrmse[t];
            if (f < 0.0) continue;                                   // repeated row or a checker failed
            ++n_valid;
            if (f > best_fit || (f == best_fit && rm < best_rmse)) {
                best_fit = f; best_rmse = rm; best = k; best_in_batch = t;
                if (P.confidence < 1.0) {
                    const double est = std::ceil(std::log(1.0 - P.confidence) / std::log(1.0 - std::pow(f, (double)P.ransac_n)));
                    if (est < (double)exit_k) exit_k = (int64_t)est;
                }
            }
        }
        if (best_in_batch >= 0) {
            GSR_HIP(hipMemcpyAsync(best_T, dT + 12 * best_in_batch, 96, hipMemcpyDeviceToHost, os.st));
            GSR_TRY(os.wait());
        }
    }
    if (best >= 0) memcpy(out->T, best_T, 96);                  // rows 0..2; row 3 is the identity's
    out->fitness = best_fit; out->inlier_rmse = best_rmse; out->best_index = best;
    out->n_evaluated = k; out->n_valid = n_valid; out->exit_index = exit_k;
    return GSR_OK;
}

// test hook: the sampler's raw draws (host code; the kernels call the same __host__ __device__ function)
int32_t gsr_debug_ransac_sample(uint64_t seed, int64_t k0, int64_t count, int64_t m, int32_t n, int32_t* out) {
    if (count < 0 || m <= 0 || m >= ((int64_t)1 << 32) || n < 1 || n > 64 || k0 < 0 || (count > 0 && !out))
        return fail(GSR_E_INVALID, "gsr_debug_ransac_sample: bad argument");
    for (int64_t t = 0; t < count; ++t)
        for (int j = 0; j < n; ++j) out[t * n + j] = (int32_t)ransac_draw(seed, (uint64_t)(k0 + t), (uint32_t)j, (uint32_t)m);
    return GSR_OK;
}

}  // extern "C"
