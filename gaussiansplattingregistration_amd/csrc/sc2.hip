// sc2.hip -- compatibility-graph global registration ("after SC2-PCR", Chen et al., CVPR 2022) on MI355X (gfx950), behind
// include/gsr_hip.h: the third global method beside RANSAC (features.hip) and FGR (fgr.hip).  DESIGN.md section 33; the float64
// NumPy model is tests/sc2_model.py.
//
//   k_sc2_gather     p_c, q_c of every correspondence once, float64; a row outside the clouds raises a flag and becomes NaN
//   k_sc2_compat     one workgroup per row i of C: 16 columns per thread and pass, one 16-byte store each; the zero padding of the
//                    row (to SC2_BK) and the zero rows behind m (to SC2_BN) are written here; deg[i] is the workgroup's integer sum
//   rocPRIM          radix sort of the keys (m - deg) << 32 | index: the first n_seeds values are the seeds in rank order
//   k_sc2_rows       the hot path: R = C[seeds, :] C^T on v_mfma_i32_32x32x32_i8, int32 out, masked by C[seed, j] in the epilogue
//   k_sc2_sets       one workgroup per seed: K1 (one walk of the row per thread, then k1 - 1 rounds of a workgroup maximum in which only
//                    the owner of the key taken walks its share again), l_j, K2 (ranks by counting),
//                    then one thread sums K2's pairs in ascending index and calls estimate_update (gsr_solve.h)
//   k_sc2_score      one workgroup per hypothesis over all m: thread t takes t, t + 256, ... ascending, the xor tree per wave, the
//                    four waves in order (gsr_fold.h)
//   refinement       k_sc2_refine_acc (block partials of the 17 Umeyama sums over the inliers), k_fold_partials, k_sc2_refine_solve,
//                    k_sc2_score on the one candidate; the host reads (good, rmse, T) and keeps or stops: one wait per step
// No floating-point atomics and no scalar memory writes: every sum has a fixed order, every discrete decision is integer arithmetic
// on C, so the same inputs give the same bits.
#include "gsr_common.h"
#include "gsr_fold.h"
#include "gsr_oneshot.h"
#include "gsr_prims.h"
#include "gsr_sc2.h"
#include "gsr_solve.h"
#include "gsr_test_hooks.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

namespace gsr {

typedef int sc2_v4i __attribute__((ext_vector_type(4)));
typedef int sc2_v16i __attribute__((ext_vector_type(16)));

// ---- correspondences --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_gather(int m, const int* __restrict__ corres, const float* __restrict__ sx, int64_t ns,
                                                          const float* __restrict__ tx, int64_t nt, double* __restrict__ P,
                                                          double* __restrict__ Q, int* __restrict__ flag) {
    for (int c = blockIdx.x * SC2_BLOCK + threadIdx.x; c < m; c += gridDim.x * SC2_BLOCK) {
        const int64_t i = corres[2 * c], j = corres[2 * c + 1];
        const bool in = i >= 0 && i < ns && j >= 0 && j < nt;
        if (!in) flag[0] = 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            P[3 * c + r] = in ? (double)sx[3 * i + r] : (double)NAN;
            Q[3 * c + r] = in ? (double)tx[3 * j + r] : (double)NAN;
        }
    }
}

__device__ __forceinline__ double sc2_len(const double a[3], const double* __restrict__ b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// Row blockIdx.x of C (ld bytes, gridDim.x = the padded row count): C_ij = 1 iff i != j and ||p_i - p_j| - |q_i - q_j|| < thr.
__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_compat(int m, int64_t ld, double thr, const double* __restrict__ P, const double* __restrict__ Q,
                                                          int8_t* __restrict__ C, int* __restrict__ deg) {
    __shared__ int s_w[SC2_BLOCK / 64];
    const int i = blockIdx.x;
    const bool live = i < m;
    double pi[3] = {0.0, 0.0, 0.0}, qi[3] = {0.0, 0.0, 0.0};
    if (live) {
#pragma unroll
        for (int r = 0; r < 3; ++r) { pi[r] = P[3 * (int64_t)i + r]; qi[r] = Q[3 * (int64_t)i + r]; }
    }
    int8_t* row = C + (int64_t)i * ld;
    int cnt = 0;
    const int groups = (int)(ld / 16);
    for (int g = threadIdx.x; g < groups; g += SC2_BLOCK) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (live) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = 16 * g + e;
                if (j < m && j != i) {
                    const double a = sc2_len(pi, P + 3 * (int64_t)j), b = sc2_len(qi, Q + 3 * (int64_t)j);
                    if (fabs(a - b) < thr) { w[e >> 2] |= 1u << (8 * (e & 3)); ++cnt; }
                }
            }
        }
        *reinterpret_cast<uint4*>(row + 16 * (int64_t)g) = make_uint4(w[0], w[1], w[2], w[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0 && live) deg[i] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_keys(int m, const int* __restrict__ deg, unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
    for (int i = blockIdx.x * SC2_BLOCK + threadIdx.x; i < m; i += gridDim.x * SC2_BLOCK) {
        key[i] = ((unsigned long long)(unsigned)(m - deg[i]) << 32) | (unsigned)i;
        val[i] = (unsigned)i;
    }
}

// ---- the i8 product ---------------------------------------------------------------------------------------------------------------
// D[r][c] = sum_k A[row(r)][k] B[c][k] for r < M, c < N, k < Kp, with row(r) = a_rows ? a_rows[r] : r; MASKED: times (A[row(r)][c] != 0).
// Both operands are K-contiguous int8 rows (lda, ldb multiples of 16, Kp a multiple of SC2_BK, both arrays zero behind their K).
// A workgroup owns a 64 x 128 tile of D: waves 0 / 1 the rows 0..31 / 32..63, waves 0,1 / 2,3 the columns 0..63 / 64..127, two 32 x 32
// accumulators per wave that share the A fragment.  A stage is 64 bytes of K: every thread brings one 16-byte piece of A and two of B
// from global memory into registers while the stage before is multiplied, then stores them to LDS rows of 80 bytes.  Lane l of the
// MFMA (r = l & 31, h = l >> 5) supplies bytes 16 h .. 16 h + 15 of the step's 32 for row r of A and for row r of B -- the SAME k for
// the same (h, byte) on both sides, which is all a sum over k needs -- and receives D[(reg & 3) + 8 (reg >> 2) + 4 h][r].
// Rows behind the arrays are never read: the row index of a load is clamped (b_rows = rows B holds), a store is guarded.
template <bool MASKED>
__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_rows(const int8_t* __restrict__ A, const int* __restrict__ a_rows, int M, int64_t lda,
                                                        const int8_t* __restrict__ B, int N, int b_rows, int64_t ldb, int Kp,
                                                        int* __restrict__ D, int64_t ldd) {
    __shared__ __attribute__((aligned(16))) int8_t s_a[SC2_BM * SC2_LDS_ROW];
    __shared__ __attribute__((aligned(16))) int8_t s_b[SC2_BN * SC2_LDS_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * SC2_BM, n0 = blockIdx.x * SC2_BN;
    const int lr = tid >> 2, lc = (tid & 3) * 16;
    int ar = m0 + lr;
    ar = ar < M ? ar : M - 1;
    const int64_t arow = a_rows ? (int64_t)a_rows[ar] : (int64_t)ar;
    int br0 = n0 + lr, br1 = n0 + 64 + lr;
    br0 = br0 < b_rows ? br0 : b_rows - 1;
    br1 = br1 < b_rows ? br1 : b_rows - 1;
    const int8_t* ga = A + arow * lda + lc;
    const int8_t* gb0 = B + (int64_t)br0 * ldb + lc;
    const int8_t* gb1 = B + (int64_t)br1 * ldb + lc;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    sc2_v16i acc0, acc1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc0[e] = 0; acc1[e] = 0; }
    sc2_v4i ra = *reinterpret_cast<const sc2_v4i*>(ga), rb0 = *reinterpret_cast<const sc2_v4i*>(gb0), rb1 = *reinterpret_cast<const sc2_v4i*>(gb1);
    for (int k0 = 0; k0 < Kp; k0 += SC2_BK) {
        __syncthreads();                                         // the stage before has been multiplied
        *reinterpret_cast<sc2_v4i*>(s_a + lr * SC2_LDS_ROW + lc) = ra;
        *reinterpret_cast<sc2_v4i*>(s_b + lr * SC2_LDS_ROW + lc) = rb0;
        *reinterpret_cast<sc2_v4i*>(s_b + (64 + lr) * SC2_LDS_ROW + lc) = rb1;
        __syncthreads();
        if (k0 + SC2_BK < Kp) {                                  // the next stage's loads fly during the MFMAs
            ra = *reinterpret_cast<const sc2_v4i*>(ga + k0 + SC2_BK);
            rb0 = *reinterpret_cast<const sc2_v4i*>(gb0 + k0 + SC2_BK);
            rb1 = *reinterpret_cast<const sc2_v4i*>(gb1 + k0 + SC2_BK);
        }
#pragma unroll
        for (int ks = 0; ks < SC2_BK / 32; ++ks) {
            const int off = ks * 32 + h * 16;
            const sc2_v4i fa = *reinterpret_cast<const sc2_v4i*>(s_a + (wm + r) * SC2_LDS_ROW + off);
            const sc2_v4i fb0 = *reinterpret_cast<const sc2_v4i*>(s_b + (wn + r) * SC2_LDS_ROW + off);
            const sc2_v4i fb1 = *reinterpret_cast<const sc2_v4i*>(s_b + (wn + 32 + r) * SC2_LDS_ROW + off);
            acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb1, acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = n0 + wn + 32 * t + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = m0 + wm + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (row < M && col < N) {
                int v = t ? acc1[e] : acc0[e];
                if (MASKED) {
                    const int64_t mrow = a_rows ? (int64_t)a_rows[row] : (int64_t)row;
                    v = A[mrow * lda + col] ? v : 0;
                }
                D[(int64_t)row * ldd + col] = v;
            }
        }
    }
}

// ---- consensus sets and hypotheses ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long sc2_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}

// Seed of rank blockIdx.x.  A candidate j (C_sj = 1) has the key (r_sj + 1) << 32 | ~j: the order (r descending, j ascending) is the
// keys descending, the keys are distinct, 0 is "none".
__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_sets(int m, int64_t ld, int k1, int k2, const unsigned* __restrict__ seeds,
                                                        const int8_t* __restrict__ C, const int* __restrict__ R, const double* __restrict__ P,
                                                        const double* __restrict__ Q, int* __restrict__ K1out, int* __restrict__ K2out,
                                                        double* __restrict__ Tout, int* __restrict__ valid) {
    __shared__ unsigned long long s_w[SC2_BLOCK / 64];
    __shared__ int s_k1[SC2_KMAX], s_l[SC2_KMAX], s_k2[SC2_KMAX], s_sorted[SC2_KMAX];
    const int tid = threadIdx.x;
    const int sidx = blockIdx.x, s = (int)seeds[sidx];
    const int* __restrict__ rrow = R + (int64_t)sidx * m;
    const int8_t* __restrict__ crow = C + (int64_t)s * ld;
    if (tid < SC2_KMAX) { s_k1[tid] = -1; s_k2[tid] = -1; s_l[tid] = 0; s_sorted[tid] = -1; }
    __syncthreads();
    if (tid == 0) s_k1[0] = s;
    // Thread t owns the candidates t, t + 256, ... and keeps the largest key among those not taken yet (`mine`).  A round is the largest
    // `mine` of the workgroup; only its owner (the keys are distinct) walks its candidates again, for its largest key below the one taken.
    // The loads do not depend on each other (R is read whether or not C says candidate), so an unrolled walk keeps them in flight.
    auto largest_below = [&](unsigned long long below) {
        unsigned long long best = 0ull;
#pragma unroll 8
        for (int j = tid; j < m; j += SC2_BLOCK) {
            const int8_t c = crow[j];
            const unsigned r = (unsigned)rrow[j];
            const unsigned long long key = c ? ((unsigned long long)(r + 1u) << 32) | (0xffffffffu - (unsigned)j) : 0ull;
            if (key < below && key > best) best = key;
        }
        return best;
    };
    unsigned long long mine = largest_below(~0ull);
    int n1 = 1;
    for (int round = 1; round < k1; ++round) {
        unsigned long long best = sc2_wave_max(mine);
        if ((tid & 63) == 0) s_w[tid >> 6] = best;
        __syncthreads();
        best = s_w[0];
#pragma unroll
        for (int w = 1; w < SC2_BLOCK / 64; ++w) best = s_w[w] > best ? s_w[w] : best;
        __syncthreads();
        if (best == 0ull) break;                                 // (the same value in every thread)
        if (tid == 0) s_k1[n1] = (int)(0xffffffffu - (unsigned)best);
        ++n1;
        if (mine == best) mine = largest_below(best);
    }
    __syncthreads();
    // l_j = how many members of K1 are compatible with member j
    if (tid < n1) {
        const int8_t* __restrict__ jrow = C + (int64_t)s_k1[tid] * ld;
        int l = 0;
        for (int k = 0; k < n1; ++k) l += jrow[s_k1[k]] ? 1 : 0;
        s_l[tid] = l;
    }
    __syncthreads();
    // K2 = s and the first k2 - 1 of the others in the order (l descending, j ascending): a member's place is how many come before it
    const int n2 = n1 < k2 ? n1 : k2;
    if (tid == 0) s_k2[0] = s;
    if (tid >= 1 && tid < n1) {
        const int lt = s_l[tid], jt = s_k1[tid];
        int before = 0;
        for (int u = 1; u < n1; ++u) before += (s_l[u] > lt || (s_l[u] == lt && s_k1[u] < jt)) ? 1 : 0;
        if (before < k2 - 1) s_k2[1 + before] = jt;
    }
    __syncthreads();
    if (tid < n2) {                                              // the members in ascending index (they are distinct)
        const int jt = s_k2[tid];
        int before = 0;
        for (int u = 0; u < n2; ++u) before += s_k2[u] < jt ? 1 : 0;
        s_sorted[before] = jt;
    }
    __syncthreads();
    if (tid < SC2_KMAX) {
        K1out[(int64_t)sidx * SC2_KMAX + tid] = s_k1[tid];
        K2out[(int64_t)sidx * SC2_KMAX + tid] = s_k2[tid];
    }
    if (tid != 0) return;
    double update[16];
    mat4_identity(update);
    bool ok = n2 >= 3;
    if (ok) {
        double acc[GSR_ICP_ACC_LEN];
        for (int e = 0; e < GSR_ICP_ACC_LEN; ++e) acc[e] = 0.0;
        acc[0] = (double)n2;
        const int64_t c0 = s_sorted[0];
        const double ctr[3] = {P[3 * c0], P[3 * c0 + 1], P[3 * c0 + 2]};
        for (int t = 0; t < n2; ++t) {
            const int64_t c = s_sorted[t];
            const double p[3] = {P[3 * c] - ctr[0], P[3 * c + 1] - ctr[1], P[3 * c + 2] - ctr[2]};
            const double q[3] = {Q[3 * c] - ctr[0], Q[3 * c + 1] - ctr[1], Q[3 * c + 2] - ctr[2]};
            for (int a = 0; a < 3; ++a) { acc[2 + a] += p[a]; acc[5 + a] += q[a]; }
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += p[a] * q[b];
        }
        estimate_update(ctr, GSR_ICP_POINT_TO_POINT, acc, update);
        for (int e = 0; e < 12; ++e) ok = ok && isfinite(update[e]);
    }
    for (int e = 0; e < 12; ++e) Tout[12 * (int64_t)sidx + e] = update[e];
    valid[sidx] = ok ? 1 : 0;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------------
// d2 of correspondence c under the rows 0..2 of a 4 x 4, as k_ransac_eval writes it
__device__ __forceinline__ double sc2_d2(const double M[12], const double* __restrict__ P, const double* __restrict__ Q, int64_t c) {
    const double px = P[3 * c], py = P[3 * c + 1], pz = P[3 * c + 2];
    const double x = M[0] * px + M[1] * py + M[2] * pz + M[3];
    const double y = M[4] * px + M[5] * py + M[6] * pz + M[7];
    const double z = M[8] * px + M[9] * py + M[10] * pz + M[11];
    const double dx = x - Q[3 * c], dy = y - Q[3 * c + 1], dz = z - Q[3 * c + 2];
    return dx * dx + dy * dy + dz * dz;
}

// good[h] = #{c : d2 < thr2} (-1 for an invalid hypothesis), rmse[h] = sqrt(sum d2 / good): hypothesis blockIdx.x over all m
__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_score(int m, double thr2, const double* __restrict__ P, const double* __restrict__ Q,
                                                         const double* __restrict__ T, const int* __restrict__ valid, int* __restrict__ good,
                                                         double* __restrict__ rmse) {
    __shared__ double s_sum[SC2_BLOCK / 64];
    __shared__ int s_cnt[SC2_BLOCK / 64];
    const int tid = threadIdx.x, hyp = blockIdx.x;
    if (!valid[hyp]) {                                           // (the whole workgroup takes this branch)
        if (tid == 0) { good[hyp] = -1; rmse[hyp] = 0.0; }
        return;
    }
    double M[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) M[e] = T[12 * (int64_t)hyp + e];
    double sum = 0.0;
    int cnt = 0;
    for (int c = tid; c < m; c += SC2_BLOCK) {
        const double d2 = sc2_d2(M, P, Q, c);
        if (d2 < thr2) { sum += d2; ++cnt; }
    }
    sum = wave_sum_xor(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sum; s_cnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        const double tot = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        const int g = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        good[hyp] = g;
        rmse[hyp] = g > 0 ? sqrt(tot / (double)g) : 0.0;
    }
}

// ---- refinement -------------------------------------------------------------------------------------------------------------------
#define SC2_NSUM 17          // n, sum d2, sum p', sum q', sum p' q'^T (p' = p - ctr, q' = q - ctr): acc[0 .. 16] of estimate_update
// Block partials over the inliers of T; thread t of block b takes the correspondences 256 b + t, + 256 grid, ... ascending.
__global__ __launch_bounds__(SC2_BLOCK) void k_sc2_refine_acc(int m, double thr2, const double* __restrict__ P, const double* __restrict__ Q,
                                                              const double* __restrict__ T, const double* __restrict__ ctr,
                                                              double* __restrict__ partials) {
    double M[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) M[e] = T[e];
    const double cx = ctr[0], cy = ctr[1], cz = ctr[2];
    double S[SC2_NSUM];
#pragma unroll
    for (int e = 0; e < SC2_NSUM; ++e) S[e] = 0.0;
    for (int c = blockIdx.x * SC2_BLOCK + threadIdx.x; c < m; c += gridDim.x * SC2_BLOCK) {
        const double d2 = sc2_d2(M, P, Q, c);
        if (d2 < thr2) {
            const double p[3] = {P[3 * (int64_t)c] - cx, P[3 * (int64_t)c + 1] - cy, P[3 * (int64_t)c + 2] - cz};
            const double q[3] = {Q[3 * (int64_t)c] - cx, Q[3 * (int64_t)c + 1] - cy, Q[3 * (int64_t)c + 2] - cz};
            S[0] += 1.0; S[1] += d2;
#pragma unroll
            for (int a = 0; a < 3; ++a) { S[2 + a] += p[a]; S[5 + a] += q[a]; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) S[8 + 3 * a + b] += p[a] * q[b];
        }
    }
    block_fold_store<SC2_NSUM, SC2_NSUM, wave_sum_xor>(S, partials, (int)blockIdx.x);
}

// Umeyama without scaling from the 17 folded sums; fewer than 3 inliers or a non-finite result: not valid
__global__ __launch_bounds__(64) void k_sc2_refine_solve(const double* __restrict__ sums, const double* __restrict__ ctr, double* __restrict__ Tnew,
                                                         int* __restrict__ valid) {
    if (threadIdx.x != 0) return;
    double acc[GSR_ICP_ACC_LEN];
    for (int e = 0; e < GSR_ICP_ACC_LEN; ++e) acc[e] = e < SC2_NSUM ? sums[e] : 0.0;
    const double c[3] = {ctr[0], ctr[1], ctr[2]};
    double update[16];
    estimate_update(c, GSR_ICP_POINT_TO_POINT, acc, update);
    bool ok = acc[0] >= 3.0;
    for (int e = 0; e < 12; ++e) ok = ok && isfinite(update[e]);
    for (int e = 0; e < 12; ++e) Tnew[e] = update[e];
    valid[0] = ok ? 1 : 0;
}

namespace {

void sc2_empty(gsr_sc2_result* out) {
    memset(out, 0, sizeof(*out));
    mat4_identity(out->T);
    out->best_seed = -1;
    out->best_index = -1;
}

bool sc2_better(int g, double r, int bg, double br) { return g > bg || (g == bg && r < br); }

// the whole method; `dbg` (test hook) receives the stages
int32_t sc2_run(const char* who, const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m64,
                const gsr_sc2_params* params, gsr_sc2_result* out, const Sc2Stages* dbg, int32_t on_device, int32_t device, void* stream) {
    if (!params || !out || ns < 0 || nt < 0 || m64 < 0) return fail(GSR_E_INVALID, "%s: bad argument", who);
    const gsr_sc2_params& O = *params;
    sc2_empty(out);
    if (!(O.seed_ratio > 0.0) || !(O.seed_ratio <= 1.0)) return fail(GSR_E_INVALID, "%s: seed_ratio must lie in (0, 1]", who);
    if (O.max_seeds < 1) return fail(GSR_E_INVALID, "%s: max_seeds must be >= 1", who);
    if (O.k2 < 3 || O.k1 < O.k2 || O.k1 > GSR_SC2_MAX_K) return fail(GSR_E_INVALID, "%s: 3 <= k2 <= k1 <= %d is required (got k1 %d, k2 %d)", who, GSR_SC2_MAX_K, O.k1, O.k2);
    if (O.refine_iters < 0) return fail(GSR_E_INVALID, "%s: refine_iters must be >= 0", who);
    if (m64 > GSR_SC2_MAX_CORRES) return fail(GSR_E_INVALID, "%s: %lld correspondences, at most %d (C is m^2 bytes)", who, (long long)m64, GSR_SC2_MAX_CORRES);
    if (m64 < 3 || !(O.d_thr > 0.0)) return GSR_OK;              // the empty result
    if (!src_xyz || !tgt_xyz || !corres) return fail(GSR_E_INVALID, "%s: NULL cloud or correspondences", who);
    if (!on_device)                                              // device arrays are checked by k_sc2_gather
        for (int64_t c = 0; c < m64; ++c)
            if (corres[2 * c] < 0 || corres[2 * c] >= ns || corres[2 * c + 1] < 0 || corres[2 * c + 1] >= nt)
                return fail(GSR_E_INVALID, "%s: correspondence %lld out of range", who, (long long)c);
    GSR_TRY(open_device(device, who));
    const int m = (int)m64;
    const int64_t ld = sc2_round_up(m, SC2_BK), mp = sc2_round_up(m, SC2_BN);
    int64_t want = (int64_t)std::ceil(O.seed_ratio * (double)m);
    const int n_seeds = (int)std::min<int64_t>(std::min<int64_t>(O.max_seeds, want), m);
    const double thr2 = O.d_thr * O.d_thr;
    // host sides of the read-backs, before `os`: it waits for the copies into them
    std::vector<int> h_good((size_t)n_seeds), h_deg((size_t)m);
    std::vector<unsigned> h_seeds((size_t)n_seeds);
    std::vector<double> h_rmse((size_t)n_seeds), h_T((size_t)n_seeds * 12);
    int h_flag = 0, h_g1 = 0;
    double h_r1 = 0.0, h_T1[12];
    DevBuf sort_tmp;                                             // rocPRIM's temporary storage: before `os`, so freed after its wait
    OneShot os((hipStream_t)stream, on_device != 0, who);
    const float *sx = nullptr, *tx = nullptr;
    const int32_t* dc = nullptr;
    double *dP = nullptr, *dQ = nullptr, *dT = nullptr, *drmse = nullptr, *dpart = nullptr, *dsums = nullptr, *dTr = nullptr, *dr1 = nullptr;
    int *dflag = nullptr, *ddeg = nullptr, *dR = nullptr, *dK1 = nullptr, *dK2 = nullptr, *dvalid = nullptr, *dgood = nullptr, *dv1 = nullptr, *dg1 = nullptr;
    int8_t* dC = nullptr;
    unsigned long long *dkey = nullptr, *dskey = nullptr;
    unsigned *dval = nullptr, *dsval = nullptr;
    GSR_TRY(os.in(src_xyz, (size_t)ns * 12, &sx));
    GSR_TRY(os.in(tgt_xyz, (size_t)nt * 12, &tx));
    GSR_TRY(os.in(corres, (size_t)m * 8, &dc));
    GSR_TRY(os.scratch((size_t)m * 24, &dP));
    GSR_TRY(os.scratch((size_t)m * 24, &dQ));
    GSR_TRY(os.scratch(4, &dflag));
    GSR_TRY(os.scratch((size_t)m * 4, &ddeg));
    GSR_TRY(os.scratch((size_t)(mp * ld), &dC));
    GSR_TRY(os.scratch((size_t)m * 8, &dkey));
    GSR_TRY(os.scratch((size_t)m * 8, &dskey));
    GSR_TRY(os.scratch((size_t)m * 4, &dval));
    GSR_TRY(os.scratch((size_t)m * 4, &dsval));
    GSR_TRY(os.scratch((size_t)n_seeds * (size_t)m * 4, &dR));
    GSR_TRY(os.scratch((size_t)n_seeds * SC2_KMAX * 4, &dK1));
    GSR_TRY(os.scratch((size_t)n_seeds * SC2_KMAX * 4, &dK2));
    GSR_TRY(os.scratch((size_t)n_seeds * 96, &dT));
    GSR_TRY(os.scratch((size_t)n_seeds * 4, &dvalid));
    GSR_TRY(os.scratch((size_t)n_seeds * 4, &dgood));
    GSR_TRY(os.scratch((size_t)n_seeds * 8, &drmse));
    GSR_TRY(os.scratch((size_t)SC2_REFINE_BLOCKS * SC2_NSUM * 8, &dpart));
    GSR_TRY(os.scratch((size_t)SC2_NSUM * 8, &dsums));
    GSR_TRY(os.scratch(2 * 96, &dTr));
    GSR_TRY(os.scratch(8, &dr1));
    GSR_TRY(os.scratch(4, &dv1));
    GSR_TRY(os.scratch(4, &dg1));
    Event ev[SC2_NSTAGE + 1];                                  // stage boundaries, recorded only for the timing hook
    const bool timed = dbg && dbg->stage_ms;
    if (timed) for (int e = 0; e <= SC2_NSTAGE; ++e) GSR_HIP(ev[e].create());
#define SC2_MARK(e) do { if (timed) GSR_HIP(hipEventRecord(ev[e], os.st)); } while (0)
    GSR_HIP(hipMemsetAsync(dflag, 0, 4, os.st));
    SC2_MARK(0);
    hipLaunchKernelGGL(k_sc2_gather, dim3(stride_grid(m, SC2_BLOCK)), dim3(SC2_BLOCK), 0, os.st, m, (const int*)dc, sx, ns, tx, nt, dP, dQ, dflag);
    hipLaunchKernelGGL(k_sc2_compat, dim3((unsigned)mp), dim3(SC2_BLOCK), 0, os.st, m, ld, O.d_thr, (const double*)dP, (const double*)dQ, dC, ddeg);
    SC2_MARK(1);
    hipLaunchKernelGGL(k_sc2_keys, dim3(stride_grid(m, SC2_BLOCK)), dim3(SC2_BLOCK), 0, os.st, m, (const int*)ddeg, dkey, dval);
    GSR_TRY((sort_pairs_by_key<rocprim::default_config>(sort_tmp, os.st, (const unsigned long long*)dkey, dskey, (const unsigned*)dval, dsval, (size_t)m, 0u, 64u)));
    SC2_MARK(2);
    hipLaunchKernelGGL(k_sc2_rows<true>, dim3((unsigned)(mp / SC2_BN), (unsigned)((n_seeds + SC2_BM - 1) / SC2_BM)), dim3(SC2_BLOCK), 0, os.st,
                       (const int8_t*)dC, (const int*)dsval, n_seeds, ld, (const int8_t*)dC, m, (int)mp, ld, (int)ld, dR, (int64_t)m);
    SC2_MARK(3);
    hipLaunchKernelGGL(k_sc2_sets, dim3((unsigned)n_seeds), dim3(SC2_BLOCK), 0, os.st, m, ld, O.k1, O.k2, (const unsigned*)dsval, (const int8_t*)dC,
                       (const int*)dR, (const double*)dP, (const double*)dQ, dK1, dK2, dT, dvalid);
    SC2_MARK(4);
    hipLaunchKernelGGL(k_sc2_score, dim3((unsigned)n_seeds), dim3(SC2_BLOCK), 0, os.st, m, thr2, (const double*)dP, (const double*)dQ, (const double*)dT,
                       (const int*)dvalid, dgood, drmse);
    SC2_MARK(5);
    GSR_HIP(hipMemcpyAsync(&h_flag, dflag, 4, hipMemcpyDeviceToHost, os.st));
    GSR_HIP(hipMemcpyAsync(h_deg.data(), ddeg, (size_t)m * 4, hipMemcpyDeviceToHost, os.st));
    GSR_HIP(hipMemcpyAsync(h_seeds.data(), dsval, (size_t)n_seeds * 4, hipMemcpyDeviceToHost, os.st));
    GSR_HIP(hipMemcpyAsync(h_good.data(), dgood, (size_t)n_seeds * 4, hipMemcpyDeviceToHost, os.st));
    GSR_HIP(hipMemcpyAsync(h_rmse.data(), drmse, (size_t)n_seeds * 8, hipMemcpyDeviceToHost, os.st));
    GSR_HIP(hipMemcpyAsync(h_T.data(), dT, (size_t)n_seeds * 96, hipMemcpyDeviceToHost, os.st));
    if (dbg) {
        if (dbg->rows) GSR_HIP(hipMemcpyAsync(dbg->rows, dR, (size_t)n_seeds * (size_t)m * 4, hipMemcpyDeviceToHost, os.st));
        if (dbg->k1) GSR_HIP(hipMemcpyAsync(dbg->k1, dK1, (size_t)n_seeds * SC2_KMAX * 4, hipMemcpyDeviceToHost, os.st));
        if (dbg->k2) GSR_HIP(hipMemcpyAsync(dbg->k2, dK2, (size_t)n_seeds * SC2_KMAX * 4, hipMemcpyDeviceToHost, os.st));
    }
    GSR_TRY(os.wait());
    int waits = 1;
    if (h_flag) return fail(GSR_E_INVALID, "%s: a correspondence row is out of range", who);
    if (dbg) {
        if (dbg->deg) memcpy(dbg->deg, h_deg.data(), (size_t)m * 4);
        if (dbg->seeds) memcpy(dbg->seeds, h_seeds.data(), (size_t)n_seeds * 4);
        if (dbg->hyp) memcpy(dbg->hyp, h_T.data(), (size_t)n_seeds * 96);
        if (dbg->good) memcpy(dbg->good, h_good.data(), (size_t)n_seeds * 4);
        if (dbg->rmse) memcpy(dbg->rmse, h_rmse.data(), (size_t)n_seeds * 8);
    }
    int64_t edges2 = 0;
    for (int i = 0; i < m; ++i) edges2 += h_deg[i];
    int best = -1, n_valid = 0;
    for (int t = 0; t < n_seeds; ++t) {
        if (h_good[t] < 0) continue;
        ++n_valid;
        if (best < 0 || sc2_better(h_good[t], h_rmse[t], h_good[best], h_rmse[best])) best = t;
    }
    out->n_seeds = n_seeds; out->n_valid = n_valid; out->n_edges = edges2 / 2; out->host_waits = waits;
    if (timed) {
        for (int e = 0; e < SC2_NSTAGE; ++e) dbg->stage_ms[e] = 0.0f;
        for (int e = 0; e < 5; ++e) GSR_HIP(hipEventElapsedTime(&dbg->stage_ms[e], ev[e], ev[e + 1]));
    }
    if (best < 0) return GSR_OK;                                 // no valid seed: the identity
    int cur_good = h_good[best];
    double cur_rmse = h_rmse[best], cur_T[12];
    memcpy(cur_T, &h_T[(size_t)best * 12], 96);
    const int64_t best_index = h_seeds[best];
    const double* dctr = dP + 3 * best_index;                    // the refinement's sums are taken about the winner's source point
    int cur = 0, steps = 0;
    if (O.refine_iters > 0) GSR_HIP(hipMemcpyAsync(dTr, dT + 12 * (int64_t)best, 96, hipMemcpyDeviceToDevice, os.st));
    const int G = (int)std::min<int64_t>((m + SC2_BLOCK - 1) / SC2_BLOCK, SC2_REFINE_BLOCKS);
    for (int it = 0; it < O.refine_iters; ++it) {
        double* Tc = dTr + 12 * cur;
        double* Tn = dTr + 12 * (1 - cur);
        hipLaunchKernelGGL(k_sc2_refine_acc, dim3(G), dim3(SC2_BLOCK), 0, os.st, m, thr2, (const double*)dP, (const double*)dQ, (const double*)Tc, dctr, dpart);
        hipLaunchKernelGGL(k_fold_partials<64>, dim3(SC2_NSUM), dim3(64), 0, os.st, (int64_t)G, SC2_NSUM, (const double*)dpart, dsums);
        hipLaunchKernelGGL(k_sc2_refine_solve, dim3(1), dim3(64), 0, os.st, (const double*)dsums, dctr, Tn, dv1);
        hipLaunchKernelGGL(k_sc2_score, dim3(1), dim3(SC2_BLOCK), 0, os.st, m, thr2, (const double*)dP, (const double*)dQ, (const double*)Tn, (const int*)dv1, dg1, dr1);
        GSR_HIP(hipMemcpyAsync(&h_g1, dg1, 4, hipMemcpyDeviceToHost, os.st));
        GSR_HIP(hipMemcpyAsync(&h_r1, dr1, 8, hipMemcpyDeviceToHost, os.st));
        GSR_HIP(hipMemcpyAsync(h_T1, Tn, 96, hipMemcpyDeviceToHost, os.st));
        GSR_TRY(os.wait());
        ++waits;
        if (h_g1 < 0 || !sc2_better(h_g1, h_r1, cur_good, cur_rmse)) break;
        cur_good = h_g1; cur_rmse = h_r1;
        memcpy(cur_T, h_T1, 96);
        cur = 1 - cur;
        ++steps;
    }
    if (timed) {                                                 // the refinement as the stream saw it, the host's decisions between its steps included
        GSR_HIP(hipEventRecord(ev[6], os.st));
        GSR_HIP(hipEventSynchronize(ev[6]));
        GSR_HIP(hipEventElapsedTime(&dbg->stage_ms[5], ev[5], ev[6]));
    }
#undef SC2_MARK
    memcpy(out->T, cur_T, 96);                                   // rows 0..2; row 3 is the identity's (every wait above is counted)
    out->fitness = (double)cur_good / (double)m;
    out->inlier_rmse = cur_rmse;
    out->best_seed = best;
    out->best_index = best_index;
    out->refine_steps = steps;
    out->host_waits = waits;
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_sc2_correspondence(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                               const gsr_sc2_params* params, gsr_sc2_result* out, int32_t on_device, int32_t device, void* stream) {
    return sc2_run("gsr_sc2_correspondence", src_xyz, ns, tgt_xyz, nt, corres, m, params, out, nullptr, on_device, device, stream);
}

// test hook: the stages of one call (host arrays)
int32_t gsr_test_sc2_stages(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                            const void* params, void* out, int32_t* deg, int32_t* seeds, int32_t* rows, int32_t* k1, int32_t* k2,
                            double* hyp, int32_t* good, double* rmse, int32_t device) {
    const Sc2Stages st = {deg, seeds, rows, k1, k2, hyp, good, rmse, nullptr};
    return sc2_run("gsr_test_sc2_stages", src_xyz, ns, tgt_xyz, nt, corres, m, (const gsr_sc2_params*)params, (gsr_sc2_result*)out, &st, 0, device, nullptr);
}

// test hook: the call itself (host or device arrays) with stream events between its stages
int32_t gsr_test_sc2_timed(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m, const void* params,
                           void* out, float* stage_ms, int32_t on_device, int32_t device, void* stream) {
    if (!stage_ms) return fail(GSR_E_INVALID, "gsr_test_sc2_timed: NULL stage_ms");
    const Sc2Stages st = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stage_ms};
    return sc2_run("gsr_test_sc2_timed", src_xyz, ns, tgt_xyz, nt, corres, m, (const gsr_sc2_params*)params, (gsr_sc2_result*)out, &st, on_device, device, stream);
}

// test hook: D = A B^T through k_sc2_rows (host arrays; the operands are copied into zero-padded device arrays of the kernel's layout)
int32_t gsr_test_i8_gemm_nt(const int8_t* A, int64_t M, const int8_t* B, int64_t N, int64_t K, int32_t* D, int32_t device) {
    if (!A || !B || !D || M < 1 || N < 1 || K < 1 || M > GSR_SC2_MAX_CORRES || N > GSR_SC2_MAX_CORRES || K > GSR_SC2_MAX_CORRES)
        return fail(GSR_E_INVALID, "gsr_test_i8_gemm_nt: bad argument");
    GSR_TRY(open_device(device, "gsr_test_i8_gemm_nt"));
    const int64_t Mp = sc2_round_up(M, SC2_BM), Np = sc2_round_up(N, SC2_BN), Kp = sc2_round_up(K, SC2_BK);
    OneShot os(nullptr, false, "gsr_test_i8_gemm_nt");
    int8_t *dA = nullptr, *dB = nullptr;
    int32_t* dD = nullptr;
    GSR_TRY(os.scratch((size_t)(Mp * Kp), &dA));
    GSR_TRY(os.scratch((size_t)(Np * Kp), &dB));
    GSR_TRY(os.out(D, (size_t)(M * N) * 4, &dD));
    GSR_HIP(hipMemsetAsync(dA, 0, (size_t)(Mp * Kp), os.st));
    GSR_HIP(hipMemsetAsync(dB, 0, (size_t)(Np * Kp), os.st));
    GSR_HIP(hipMemcpy2DAsync(dA, (size_t)Kp, A, (size_t)K, (size_t)K, (size_t)M, hipMemcpyHostToDevice, os.st));
    GSR_HIP(hipMemcpy2DAsync(dB, (size_t)Kp, B, (size_t)K, (size_t)K, (size_t)N, hipMemcpyHostToDevice, os.st));
    hipLaunchKernelGGL(k_sc2_rows<false>, dim3((unsigned)(Np / SC2_BN), (unsigned)(Mp / SC2_BM)), dim3(SC2_BLOCK), 0, os.st, (const int8_t*)dA,
                       (const int*)nullptr, (int)M, Kp, (const int8_t*)dB, (int)N, (int)Np, Kp, (int)Kp, (int*)dD, N);
    return os.finish();
}

}  // extern "C"
