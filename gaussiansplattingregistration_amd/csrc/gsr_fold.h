// gsr_fold.h -- the fixed-order float64 fold.  Device only.  Every registration method returns float64 sums
// that come out with the same bits on every run and every launch shape, because the order of summation is fixed:
//   1. a lane adds its rows in ascending order (the caller's loop);
//   2. the 64 lanes of a wave are combined in a fixed tree: wave_sum_xor or wave_sum_rows -- the two trees give DIFFERENT bits, every
//      caller keeps the one it has;
//   3. the four waves of a 256-thread block are added as ((w0 + w1) + w2) + w3 (block_fold_store);
//   4. a second kernel gives thread t the block partials t, t + THREADS, ... in ascending order and finishes with the xor tree (and,
//      with four waves, step 3 again): k_fold_partials.
// tests/fold_model.py restates 2 to 4 in NumPy; tests/test_fold_gpu.py holds this header to it bit for bit.
#pragma once
#include "gsr_common.h"

namespace gsr {

// The butterfly over lanes l ^ 32, 16, 8, 4, 2, 1 in that order; every lane gets the sum.
__device__ __forceinline__ double wave_sum_xor(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Sum of a double over the 64 lanes (every lane gets it) in a fixed order, without the LDS crossbar: four DPP row rotations
// and the two permlane swaps, on the two dwords of the value.  (30 accumulators x 6 steps of __shfl_xor were 360
// ds_bpermute per wave, 24 LDS-pipe cycles each: a third of the accumulate kernel on a 185 k-point level.)
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
template <bool HALF>        // HALF: lanes l and l ^ 32, else l and l ^ 16
__device__ __forceinline__ double swap_sum_d(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const auto rl = HALF ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false) : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = HALF ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false) : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const double a = __builtin_bit_cast(double, ((long long)(unsigned)rh[0] << 32) | (unsigned)rl[0]);
    const double c = __builtin_bit_cast(double, ((long long)(unsigned)rh[1] << 32) | (unsigned)rl[1]);
    return a + c;
}
// Rows of 16 lanes first: the butterfly over lanes l ^ 8, 4, 2, 1, then 16, then 32.  (A rotation by r within a row of 16 meets
// lane l ^ r's value here, because after the step before it the values repeat with period 2 r.)
__device__ __forceinline__ double wave_sum_rows(double v) {
    v += dpp_d<0x128>(v);       // row_ror:8
    v += dpp_d<0x124>(v);       // row_ror:4
    v += dpp_d<0x122>(v);       // row_ror:2
    v += dpp_d<0x121>(v);       // row_ror:1
    v = swap_sum_d<false>(v);
    v = swap_sum_d<true>(v);
    return v;
}

// The block's share of NACC sums, for 256-thread blocks: partials[row * STRIDE + k] = ((s0 + s1) + s2) + s3 with s_w = WaveSum of
// acc[k] over wave w.  Every thread of the block must call it (it holds a barrier).
template <int NACC, int STRIDE, double (*WaveSum)(double)>
__device__ __forceinline__ void block_fold_store(double (&acc)[NACC], double* __restrict__ partials, int row) {
    static_assert(NACC <= STRIDE && NACC <= 256, "block_fold_store: a thread per sum, NACC sums in a row of STRIDE");
    __shared__ double s_red[4][NACC];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double v = WaveSum(acc[k]);
        if (lane == 0) s_red[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        const int k = threadIdx.x;
        const double v = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
        partials[(int64_t)row * STRIDE + k] = v;
    }
}

// out[k] = the sum of partials[b * stride + k] over the nblocks blocks, one group of THREADS per sum k = blockIdx.x: thread t adds
// the blocks t, t + THREADS, ... in ascending order, then the xor tree per wave; with 256 threads the four waves in order (a single
// wavefront walks a chain of dependent loads four times as long: worth it where the blocks are many, as the tiles of an image are).
template <int THREADS>
static __global__ __launch_bounds__(THREADS) void k_fold_partials(int64_t nblocks, int stride, const double* __restrict__ partials, double* __restrict__ out) {
    static_assert(THREADS == 64 || THREADS == 256, "k_fold_partials: one wave or four");
    const int k = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int64_t b = t; b < nblocks; b += THREADS) s += partials[b * stride + k];
    s = wave_sum_xor(s);
    if constexpr (THREADS == 64) {
        if (t == 0) out[k] = s;
    } else {
        __shared__ double s_w[4];
        if ((t & 63) == 0) s_w[t >> 6] = s;
        __syncthreads();
        if (t == 0) out[k] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    }
}

}  // namespace gsr
