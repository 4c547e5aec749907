// fgr.hip -- Fast Global Registration on MI355X (gfx950), behind include/gsr_hip.h: the second method of the reference's "Global"
// tab (do_fgr_registration) as Open3D 0.16 FastGlobalRegistration.cpp runs it.  DESIGN.md section 12.
//
//   gsr_fgr_tuple_test  k_fgr_tuple (a trial per thread: three counter-based draws, six gathers, six float64 lengths, the flag, the
//                       block's count), k_fgr_tuple_scan (one block: exclusive scan of the block counts) and k_fgr_tuple_emit (ballot +
//                       mbcnt rank within the wave, wave offsets within the block: the accepted trials land in trial order); the host
//                       reads one count per batch and stops at maximum_tuple_count
//   gsr_fgr_optimize    k_fgr_centre_* / k_fgr_norm_partial / k_fgr_init (two-stage fixed-order float64 sums and a max), k_fgr_gather
//                       (normalised p_c, q_c as struct-of-arrays float64), then per iteration k_fgr_accumulate (block partials of the
//                       16 distinct sums behind JTJ and JTr) and k_fgr_step (folds them in block order; one thread solves, composes,
//                       anneals mu and leaves delta for the next accumulate).  All iterations are enqueued at once: one stream wait.
// No floating-point atomics: every sum has a fixed order, so the same inputs give the same bits.
#include "gsr_common.h"
#include "gsr_features.h"
#include "gsr_fold.h"
#include "gsr_oneshot.h"
#include "gsr_solve.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <cmath>

namespace gsr {

#define FGR_BLOCK 256
#define FGR_WAVES (FGR_BLOCK / 64)
#define FGR_NSUM 16          // distinct sums behind the 21 + 6 entries of JTJ and JTr (the J rows are sparse)
#define FGR_MAX_BLOCKS 256   // block partials the single-block fold of k_fgr_step / k_fgr_centre_fold / k_fgr_init walks

// ---- tuple test ----------------------------------------------------------------------------------------------------------------
struct FgrTupleArgs {
    int64_t k0;              // first trial of the batch
    int nb;                  // trials in the batch
    uint32_t m;
    uint64_t seed;
    double s;
    int64_t ns, nt;
};
// info[0] = accepted trials of the batch (k_fgr_tuple_scan), info[1] = 1 if a correspondence row was out of range,
// info[2] = trial index of the accepted trial that filled the list

__device__ __forceinline__ double edge_len(const float* __restrict__ x, int64_t a, int64_t b) {
    const double dx = (double)x[3 * a] - (double)x[3 * b], dy = (double)x[3 * a + 1] - (double)x[3 * b + 1], dz = (double)x[3 * a + 2] - (double)x[3 * b + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// flag[t] = 1 iff trial k0 + t passes; bcount[block] = how many of the block's trials pass.
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_tuple(FgrTupleArgs a, const float* __restrict__ sx, const float* __restrict__ tx,
                                                         const int* __restrict__ corres, unsigned char* __restrict__ flag,
                                                         int* __restrict__ bcount, int64_t* __restrict__ info) {
    __shared__ int s_w[FGR_WAVES];
    const int t = blockIdx.x * FGR_BLOCK + threadIdx.x;
    bool ok = false;
    if (t < a.nb) {
        int64_t i[3], j[3];
        bool in = true;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int64_t r = ransac_draw(a.seed, (uint64_t)(a.k0 + t), (uint32_t)e, a.m);
            i[e] = corres[2 * r];
            j[e] = corres[2 * r + 1];
            in = in && i[e] >= 0 && i[e] < a.ns && j[e] >= 0 && j[e] < a.nt;
        }
        if (in) {
            ok = true;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int f = e == 2 ? 0 : e + 1;
                const double li = edge_len(sx, i[e], i[f]), lj = edge_len(tx, j[e], j[f]);
                ok = ok && (li * a.s < lj) && (lj < li / a.s);
            }
        } else {
            info[1] = 1;
        }
        flag[t] = ok ? 1 : 0;
    }
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < FGR_WAVES; ++w) c += s_w[w];
        bcount[blockIdx.x] = c;
    }
}

// boff[b] = sum of bcount[0 .. b), info[0] = the total.  One block: a contiguous run of blocks per thread, then a scan of the 256 runs.
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_tuple_scan(int nblk, const int* __restrict__ bcount, int* __restrict__ boff,
                                                              int64_t* __restrict__ info) {
    __shared__ int s_run[FGR_BLOCK];
    const int tid = threadIdx.x;
    const int per = (nblk + FGR_BLOCK - 1) / FGR_BLOCK;
    const int lo = tid * per, hi = lo + per < nblk ? lo + per : nblk;
    int run = 0;
    for (int b = lo; b < hi; ++b) run += bcount[b];
    s_run[tid] = run;
    __syncthreads();
    for (int d = 1; d < FGR_BLOCK; d <<= 1) {                       // inclusive Hillis-Steele scan (integers: any order is exact)
        const int v = tid >= d ? s_run[tid - d] : 0;
        __syncthreads();
        s_run[tid] += v;
        __syncthreads();
    }
    int off = s_run[tid] - run;
    for (int b = lo; b < hi; ++b) { boff[b] = off; off += bcount[b]; }
    if (tid == FGR_BLOCK - 1) info[0] = s_run[tid];
}

// The accepted trial of global rank g = taken + (accepted trials before it in the batch) writes its three pairs to out[6 g ..] while
// g < max_tuple: trial order, whatever the batch size.
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_tuple_emit(FgrTupleArgs a, const int* __restrict__ corres, const unsigned char* __restrict__ flag,
                                                              const int* __restrict__ boff, int64_t taken, int64_t max_tuple,
                                                              int* __restrict__ out, int64_t* __restrict__ info) {
    __shared__ int s_w[FGR_WAVES];
    const int t = blockIdx.x * FGR_BLOCK + threadIdx.x;
    const bool ok = t < a.nb && flag[t] != 0;
    const unsigned long long b = __ballot(ok);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int before = boff[blockIdx.x];
    for (int w = 0; w < wave; ++w) before += s_w[w];
    const int64_t g = taken + before + rank;
    if (ok && g < max_tuple) {
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int64_t r = ransac_draw(a.seed, (uint64_t)(a.k0 + t), (uint32_t)e, a.m);
            out[6 * g + 2 * e] = corres[2 * r];
            out[6 * g + 2 * e + 1] = corres[2 * r + 1];
        }
        if (g == max_tuple - 1) info[2] = a.k0 + t;
    }
}

// ---- normalisation -------------------------------------------------------------------------------------------------------------
struct FgrState {
    double trans[16];        // the accumulated transform (target -> source, normalised units)
    double delta[12];        // rows 0..2 of the last update: the next k_fgr_accumulate applies it to q
    double mean[6];          // source, target
    double scale, scale_global, mu;
    int iterations, done, bad_rows, pad;
};

// the largest value of the wave by a fixed shuffle tree (lane 0 holds it)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}

// part[(cloud * G + block) * 3 + r] = the block's share of sum x_r of cloud blockIdx.y (0 source, 1 target): thread t takes the points
// block * 256 + t, + g * 256, ... in ascending order
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_centre_partial(const float* __restrict__ sx, int64_t ns, const float* __restrict__ tx, int64_t nt,
                                                                  double* __restrict__ part) {
    const float* x = blockIdx.y ? tx : sx;
    const int64_t n = blockIdx.y ? nt : ns;
    // the cloud's own block count g = min(ceil(n / 256), grid): its order of summation does not depend on the other cloud's size
    int64_t g = (n + FGR_BLOCK - 1) / FGR_BLOCK;
    g = g < 1 ? 1 : (g > (int64_t)gridDim.x ? (int64_t)gridDim.x : g);
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x; i < n && blockIdx.x < g; i += g * FGR_BLOCK) {
        s[0] += (double)x[3 * i]; s[1] += (double)x[3 * i + 1]; s[2] += (double)x[3 * i + 2];
    }
    block_fold_store<3, 3, wave_sum_xor>(s, part, (int)(blockIdx.y * gridDim.x + blockIdx.x));
}

// mean[cloud * 3 + r] = (the block partials in block order) / n
__global__ __launch_bounds__(64) void k_fgr_centre_fold(int G, const double* __restrict__ part, int64_t ns, int64_t nt, FgrState* __restrict__ st) {
    const int t = threadIdx.x;
    if (t >= 6) return;
    const int cloud = t / 3, r = t % 3;
    double s = 0.0;
    for (int b = 0; b < G; ++b) s += part[((int64_t)cloud * G + b) * 3 + r];
    st->mean[t] = s / (double)(cloud ? nt : ns);
}

// pmax[cloud * G + block] = the largest squared norm of a centred point among the block's points
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_norm_partial(const float* __restrict__ sx, int64_t ns, const float* __restrict__ tx, int64_t nt,
                                                                const FgrState* __restrict__ st, double* __restrict__ pmax) {
    __shared__ double s_w[FGR_WAVES];
    const float* x = blockIdx.y ? tx : sx;
    const int64_t n = blockIdx.y ? nt : ns;
    const double mx = st->mean[3 * blockIdx.y], my = st->mean[3 * blockIdx.y + 1], mz = st->mean[3 * blockIdx.y + 2];
    double best = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FGR_BLOCK) {
        const double dx = (double)x[3 * i] - mx, dy = (double)x[3 * i + 1] - my, dz = (double)x[3 * i + 2] - mz;
        best = fmax(best, (dx * dx + dy * dy) + dz * dz);
    }
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < FGR_WAVES; ++w) best = fmax(best, s_w[w]);
        pmax[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = best;
    }
}

// scale, scale_global, the first mu, trans = delta = identity
__global__ __launch_bounds__(64) void k_fgr_init(int G, const double* __restrict__ pmax, int use_absolute_scale, FgrState* __restrict__ st) {
    if (threadIdx.x != 0) return;
    double best = 0.0;
    for (int b = 0; b < 2 * G; ++b) best = fmax(best, pmax[b]);
    const double scale = sqrt(best);
    st->scale = scale;
    st->scale_global = use_absolute_scale ? 1.0 : scale;
    st->mu = use_absolute_scale ? scale : 1.0;
    for (int e = 0; e < 16; ++e) st->trans[e] = (e % 5 == 0) ? 1.0 : 0.0;
    for (int e = 0; e < 12; ++e) st->delta[e] = (e % 5 == 0) ? 1.0 : 0.0;
    st->iterations = 0; st->done = 0; st->bad_rows = 0; st->pad = 0;
}

// pq[r * m + c] = normalised source coordinate r of pair c, pq[(3 + r) * m + c] = its target coordinate
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_gather(int64_t m, const int* __restrict__ corres, const float* __restrict__ sx, int64_t ns,
                                                          const float* __restrict__ tx, int64_t nt, FgrState* __restrict__ st, double* __restrict__ pq) {
    const double sg = st->scale_global;
    for (int64_t c = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x; c < m; c += (int64_t)gridDim.x * FGR_BLOCK) {
        const int64_t i = corres[2 * c], j = corres[2 * c + 1];
        const bool in = i >= 0 && i < ns && j >= 0 && j < nt;
        if (!in) st->bad_rows = 1;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            pq[r * m + c] = in ? ((double)sx[3 * i + r] - st->mean[r]) / sg : 0.0;
            pq[(3 + r) * m + c] = in ? ((double)tx[3 * j + r] - st->mean[3 + r]) / sg : 0.0;
        }
    }
}

// ---- optimisation --------------------------------------------------------------------------------------------------------------
// One iteration's sums.  With q = (x, y, z) (after the previous update), r = p - q and l = (mu / (r.r + mu))^2 the rows
// J0 = [0, -z, y, -1, 0, 0], J1 = [z, 0, -x, 0, -1, 0], J2 = [-y, x, 0, 0, 0, -1] give
//   JTJ = l * [[yy+zz, -xy, -xz, 0, -z, y], [., xx+zz, -yz, z, 0, -x], [., ., xx+yy, -y, x, 0], [., ., ., 1, 0, 0], [.., 1, 0], [.., 1]]
//   JTr = l * [z ry - y rz, x rz - z rx, y rx - x ry, -rx, -ry, -rz]
// so 16 sums carry all 27 entries: S0..5 = l (yy+zz, xy, xz, xx+zz, yz, xx+yy), S6..8 = l (x, y, z), S9 = l, S10..15 = JTr.
// Thread t takes the pairs block * 256 + t, + grid * 256, ... in ascending order; block_fold_store (gsr_fold.h, the xor tree); partials[block][16].
__global__ __launch_bounds__(FGR_BLOCK) void k_fgr_accumulate(int64_t m, double* __restrict__ pq, const FgrState* __restrict__ st,
                                                              double* __restrict__ partials) {
    if (st->done) return;
    double D[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) D[e] = st->delta[e];
    const double mu = st->mu;
    double S[FGR_NSUM];
#pragma unroll
    for (int e = 0; e < FGR_NSUM; ++e) S[e] = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * FGR_BLOCK + threadIdx.x; c < m; c += (int64_t)gridDim.x * FGR_BLOCK) {
        const double px = pq[c], py = pq[m + c], pz = pq[2 * m + c];
        const double ox = pq[3 * m + c], oy = pq[4 * m + c], oz = pq[5 * m + c];
        const double x = D[0] * ox + D[1] * oy + D[2] * oz + D[3];
        const double y = D[4] * ox + D[5] * oy + D[6] * oz + D[7];
        const double z = D[8] * ox + D[9] * oy + D[10] * oz + D[11];
        pq[3 * m + c] = x; pq[4 * m + c] = y; pq[5 * m + c] = z;
        const double rx = px - x, ry = py - y, rz = pz - z;
        const double w = mu / (rx * rx + ry * ry + rz * rz + mu);
        const double l = w * w;
        S[0] += l * (y * y + z * z); S[1] += l * (x * y); S[2] += l * (x * z);
        S[3] += l * (x * x + z * z); S[4] += l * (y * z); S[5] += l * (x * x + y * y);
        S[6] += l * x; S[7] += l * y; S[8] += l * z; S[9] += l;
        S[10] += l * (z * ry - y * rz); S[11] += l * (x * rz - z * rx); S[12] += l * (y * rx - x * ry);
        S[13] -= l * rx; S[14] -= l * ry; S[15] -= l * rz;
    }
    block_fold_store<FGR_NSUM, FGR_NSUM, wave_sum_xor>(S, partials, (int)blockIdx.x);
}

// Folds the block partials in block order (a sum per thread), then thread 0: (-JTJ) x = JTr, delta, trans = delta trans, mu.
__global__ __launch_bounds__(64) void k_fgr_step(int nblk, const double* __restrict__ partials, int decrease_mu, double division_factor,
                                                 double max_corr, FgrState* __restrict__ st) {
    __shared__ double s_sum[FGR_NSUM];
    if (st->done) return;
    if (threadIdx.x < FGR_NSUM) {
        double v = 0.0;
        for (int b = 0; b < nblk; ++b) v += partials[(int64_t)b * FGR_NSUM + threadIdx.x];
        s_sum[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double S[FGR_NSUM];
#pragma unroll
    for (int e = 0; e < FGR_NSUM; ++e) S[e] = s_sum[e];
    double A[6][6], b[6], x[6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) A[r][c] = 0.0;
    A[0][0] = -S[0]; A[0][1] = S[1];  A[0][2] = S[2];  A[0][4] = S[8];  A[0][5] = -S[7];
    A[1][1] = -S[3]; A[1][2] = S[4];  A[1][3] = -S[8]; A[1][5] = S[6];
    A[2][2] = -S[5]; A[2][3] = S[7];  A[2][4] = -S[6];
    A[3][3] = -S[9]; A[4][4] = -S[9]; A[5][5] = -S[9];
#pragma unroll
    for (int r = 1; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < r; ++c) A[r][c] = A[c][r];
#pragma unroll
    for (int r = 0; r < 6; ++r) b[r] = S[10 + r];
    solve6(A, b, x);
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) ok = ok && isfinite(x[r]);
    if (!ok) { st->done = 1; return; }
    double d[16];
    rigid_from_euler6(x, d);
    double T[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = st->trans[e];
    mat4_mul(d, T, T);
#pragma unroll
    for (int e = 0; e < 16; ++e) st->trans[e] = T[e];
#pragma unroll
    for (int e = 0; e < 12; ++e) st->delta[e] = d[e];
    const int itr = st->iterations;
    const double mu = st->mu;
    if (decrease_mu && itr % 4 == 0 && mu > max_corr) st->mu = mu / division_factor;
    st->iterations = itr + 1;
}

namespace {

int fgr_grid(int64_t n) {
    int64_t g = (n + FGR_BLOCK - 1) / FGR_BLOCK;
    if (g < 1) g = 1;
    if (g > FGR_MAX_BLOCKS) g = FGR_MAX_BLOCKS;
    return (int)g;
}

int32_t check_common(const char* who, const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                     const gsr_fgr_options* o, int32_t on_device) {
    if (!o) return fail(GSR_E_INVALID, "%s: NULL options", who);
    if (ns < 0 || nt < 0 || m < 0) return fail(GSR_E_INVALID, "%s: negative count", who);
    if (m >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "%s: too many correspondences", who);
    if (m > 0 && (!src_xyz || !tgt_xyz || !corres)) return fail(GSR_E_INVALID, "%s: NULL cloud or correspondences", who);
    if (!on_device)       // device arrays are checked by the kernels
        for (int64_t c = 0; c < m; ++c)
            if (corres[2 * c] < 0 || corres[2 * c] >= ns || corres[2 * c + 1] < 0 || corres[2 * c + 1] >= nt)
                return fail(GSR_E_INVALID, "%s: correspondence %lld out of range", who, (long long)c);
    return GSR_OK;
}

// the inverse of the affine map [A | t] (rows 0..2 of M), row-major 4x4
bool invert_affine(const double M[16], double out[16]) {
    const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], i = M[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (!(fabs(det) > 0.0) || !std::isfinite(det)) return false;
    const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                           (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                           (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
    for (int r = 0; r < 3; ++r) {
        for (int col = 0; col < 3; ++col) out[4 * r + col] = inv[3 * r + col];
        out[4 * r + 3] = -(inv[3 * r] * M[3] + inv[3 * r + 1] * M[7] + inv[3 * r + 2] * M[11]);
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
    return true;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_fgr_tuple_test(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                           const gsr_fgr_options* options, int32_t* corres_out, int64_t* n_out, int64_t* n_trials, int32_t on_device,
                           int32_t device, void* stream) {
    if (!n_out || !n_trials) return fail(GSR_E_INVALID, "gsr_fgr_tuple_test: NULL count");
    *n_out = 0; *n_trials = 0;
    GSR_TRY(check_common("gsr_fgr_tuple_test", src_xyz, ns, tgt_xyz, nt, corres, m, options, on_device));
    const gsr_fgr_options& O = *options;
    if (O.maximum_tuple_count < 0) return fail(GSR_E_INVALID, "gsr_fgr_tuple_test: maximum_tuple_count must be >= 0");
    if (!(O.tuple_scale > 0.0) || !std::isfinite(O.tuple_scale)) return fail(GSR_E_INVALID, "gsr_fgr_tuple_test: tuple_scale must be > 0");
    if (m == 0 || O.maximum_tuple_count == 0) return GSR_OK;
    if (!corres_out) return fail(GSR_E_INVALID, "gsr_fgr_tuple_test: NULL corres_out");
    GSR_TRY(open_device(device, "gsr_fgr_tuple_test"));
    const int64_t total = 100 * m, max_tuple = O.maximum_tuple_count;
    int64_t B = O.batch > 0 ? O.batch : 65536;
    if (B > (1 << 20)) B = 1 << 20;
    if (B > total) B = total;
    const int nblk_max = (int)((B + FGR_BLOCK - 1) / FGR_BLOCK);
    int64_t h_info[3] = {0, 0, 0};                               // before `os`: it waits for the copies into it
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_fgr_tuple_test");
    const float *sx = nullptr, *tx = nullptr;
    const int32_t* dc = nullptr;
    int32_t* dout = nullptr;
    unsigned char* dflag = nullptr;
    int *dcount = nullptr, *doff = nullptr;
    int64_t* dinfo = nullptr;
    GSR_TRY(os.in(src_xyz, (size_t)ns * 12, &sx));
    GSR_TRY(os.in(tgt_xyz, (size_t)nt * 12, &tx));
    GSR_TRY(os.in(corres, (size_t)m * 8, &dc));
    GSR_TRY(os.out(corres_out, (size_t)max_tuple * 24, &dout));
    GSR_TRY(os.scratch((size_t)B, &dflag));
    GSR_TRY(os.scratch((size_t)nblk_max * 4, &dcount));
    GSR_TRY(os.scratch((size_t)nblk_max * 4, &doff));
    GSR_TRY(os.scratch(24, &dinfo));
    GSR_HIP(hipMemsetAsync(dinfo, 0, 24, os.st));
    if (!on_device) GSR_HIP(hipMemsetAsync(dout, 0, (size_t)max_tuple * 24, os.st));     // the unused tail goes back to the caller
    FgrTupleArgs a;
    a.m = (uint32_t)m; a.seed = O.seed; a.s = O.tuple_scale; a.ns = ns; a.nt = nt;
    int64_t taken = 0, k = 0, visited = total;
    while (k < total && taken < max_tuple) {
        a.k0 = k; a.nb = (int)std::min<int64_t>(B, total - k);
        const int nblk = (a.nb + FGR_BLOCK - 1) / FGR_BLOCK;
        hipLaunchKernelGGL(k_fgr_tuple, dim3(nblk), dim3(FGR_BLOCK), 0, os.st, a, sx, tx, (const int*)dc, dflag, dcount, dinfo);
        hipLaunchKernelGGL(k_fgr_tuple_scan, dim3(1), dim3(FGR_BLOCK), 0, os.st, nblk, (const int*)dcount, doff, dinfo);
        hipLaunchKernelGGL(k_fgr_tuple_emit, dim3(nblk), dim3(FGR_BLOCK), 0, os.st, a, (const int*)dc, (const unsigned char*)dflag, (const int*)doff, taken,
                           max_tuple, (int*)dout, dinfo);
        GSR_HIP(hipMemcpyAsync(h_info, dinfo, 24, hipMemcpyDeviceToHost, os.st));
        GSR_TRY(os.wait());
        if (h_info[1]) return fail(GSR_E_INVALID, "gsr_fgr_tuple_test: a correspondence row is out of range");
        if (taken + h_info[0] >= max_tuple) { taken = max_tuple; visited = h_info[2] + 1; break; }
        taken += h_info[0];
        k += a.nb;
    }
    GSR_TRY(os.finish());
    *n_out = 3 * taken;
    *n_trials = visited;
    return GSR_OK;
}

int32_t gsr_fgr_optimize(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                         const gsr_fgr_options* options, gsr_fgr_result* result, int32_t on_device, int32_t device, void* stream) {
    if (!result) return fail(GSR_E_INVALID, "gsr_fgr_optimize: NULL result");
    mat4_identity(result->T);
    result->n_corres = 0; result->iterations = 0; result->host_waits = 0; result->scale_global = 0.0;
    GSR_TRY(check_common("gsr_fgr_optimize", src_xyz, ns, tgt_xyz, nt, corres, m, options, on_device));
    const gsr_fgr_options& O = *options;
    if (ns == 0 || nt == 0 || !src_xyz || !tgt_xyz) return fail(GSR_E_INVALID, "gsr_fgr_optimize: empty cloud");
    if (O.iteration_number < 0) return fail(GSR_E_INVALID, "gsr_fgr_optimize: iteration_number must be >= 0");
    if (O.decrease_mu && !(O.division_factor > 0.0)) return fail(GSR_E_INVALID, "gsr_fgr_optimize: division_factor must be > 0");
    GSR_TRY(open_device(device, "gsr_fgr_optimize"));
    FgrState h;                                                  // before `os`: it waits for the copy into it
    memset(&h, 0, sizeof(h));
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_fgr_optimize");
    const float *sx = nullptr, *tx = nullptr;
    const int32_t* dc = nullptr;
    double *part = nullptr, *pmax = nullptr, *pq = nullptr, *partials = nullptr;
    FgrState* st = nullptr;
    const int G = fgr_grid(std::max(ns, nt));
    const bool run = m >= 10;
    const int nblk = fgr_grid(m);
    GSR_TRY(os.in(src_xyz, (size_t)ns * 12, &sx));
    GSR_TRY(os.in(tgt_xyz, (size_t)nt * 12, &tx));
    GSR_TRY(os.in(corres, (size_t)m * 8, &dc));
    GSR_TRY(os.scratch((size_t)2 * G * 3 * 8, &part));
    GSR_TRY(os.scratch((size_t)2 * G * 8, &pmax));
    GSR_TRY(os.scratch(sizeof(FgrState), &st));
    hipLaunchKernelGGL(k_fgr_centre_partial, dim3(G, 2), dim3(FGR_BLOCK), 0, os.st, sx, ns, tx, nt, part);
    hipLaunchKernelGGL(k_fgr_centre_fold, dim3(1), dim3(64), 0, os.st, G, (const double*)part, ns, nt, st);
    hipLaunchKernelGGL(k_fgr_norm_partial, dim3(G, 2), dim3(FGR_BLOCK), 0, os.st, sx, ns, tx, nt, (const FgrState*)st, pmax);
    hipLaunchKernelGGL(k_fgr_init, dim3(1), dim3(64), 0, os.st, G, (const double*)pmax, O.use_absolute_scale ? 1 : 0, st);
    if (run) {
        GSR_TRY(os.scratch((size_t)m * 48, &pq));
        GSR_TRY(os.scratch((size_t)nblk * FGR_NSUM * 8, &partials));
        hipLaunchKernelGGL(k_fgr_gather, dim3(nblk), dim3(FGR_BLOCK), 0, os.st, m, (const int*)dc, sx, ns, tx, nt, st, pq);
        for (int it = 0; it < O.iteration_number; ++it) {
            hipLaunchKernelGGL(k_fgr_accumulate, dim3(nblk), dim3(FGR_BLOCK), 0, os.st, m, pq, (const FgrState*)st, partials);
            hipLaunchKernelGGL(k_fgr_step, dim3(1), dim3(64), 0, os.st, nblk, (const double*)partials, O.decrease_mu ? 1 : 0, O.division_factor,
                               O.maximum_correspondence_distance, st);
        }
    }
    GSR_HIP(hipMemcpyAsync(&h, st, sizeof(FgrState), hipMemcpyDeviceToHost, os.st));
    GSR_TRY(os.wait());                                          // the only wait of the call
    if (h.bad_rows) return fail(GSR_E_INVALID, "gsr_fgr_optimize: a correspondence row is out of range");
    result->n_corres = m;
    result->iterations = h.iterations;
    result->host_waits = 1;
    result->scale_global = h.scale_global;
    if (!run) return GSR_OK;
    // back to the caller's units: M = [R | -R mean_t + t scale_global + mean_s] aligns the target with the source; T = M^-1
    double M[16];
    memcpy(M, h.trans, sizeof(M));
    for (int r = 0; r < 3; ++r) {
        double v = 0.0;
        for (int c = 0; c < 3; ++c) v += h.trans[4 * r + c] * h.mean[3 + c];
        M[4 * r + 3] = -v + h.trans[4 * r + 3] * h.scale_global + h.mean[r];
    }
    double T[16];
    if (!invert_affine(M, T)) return fail(GSR_E_PRECONDITION, "gsr_fgr_optimize: the optimised transform is singular or not finite");
    memcpy(result->T, T, sizeof(T));
    return GSR_OK;
}

}  // extern "C"
