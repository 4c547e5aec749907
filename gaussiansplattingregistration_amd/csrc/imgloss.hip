// imgloss.hip -- the photometric loss of the fine-tuner, (1 - lambda) L1 + lambda (1 - SSIM), and its gradient with respect to the
// image in ONE kernel (gsr_loss_*).  DESIGN.md section 29; the contract is in include/gsr_hip.h; tests/ssim_loss_model.py restates
// it, operation by operation, in NumPy.
//
// k_loss_tiles<GRAD>: one 256-thread group per 16 x 16 tile of the (H, W, 3) image, the three channels one after the other in the
// same LDS.  Per channel:
//   1. the tile with a halo of 10 pixels (5 without the gradient) of both images goes to LDS, zeros outside the image;
//   2. a horizontal 11-tap pass leaves the five moment rows (a, b, a a, b b, a b) in LDS;
//   3. the vertical pass gives every pixel of the tile +- 5 its five moments, and from them its SSIM term S and the three derivative
//      maps D1, D2, D3 (zero where the pixel is outside the image), which go to LDS.  Thread t takes its OWN pixel (t & 15, t >> 4)
//      first -- so S stays in a register for the sums -- and then the 420 pixels of the ring around the tile;
//   4. a horizontal pass over D1, D2, D3 (into the space of the moment rows, which are dead by then);
//   5. the vertical pass, the pointwise combination with a and b, ONE rounding to float32, the store.
// Everything between the float32 loads and that store is float64 and nothing image-sized is written but the gradient.  Every
// thread adds |a - b| and S of its own pixel over the channels in ascending order; block_fold_store and k_fold_partials<256> fold
// them (gsr_fold.h): no atomics, the same inputs give the same bits.  Without the gradient the same arithmetic runs on the tile +- 5
// only, so the three outputs have the same bits either way.
#include "gsr_common.h"
#include "gsr_fold.h"
#include "gsr_oneshot.h"
#include "gsr_ssim_window.h"

using namespace gsr;

namespace {

constexpr int LT = 16;                              // the tile
constexpr int RAD = SSIM_WIN / 2;                   // 5
constexpr int MID = LT + 2 * RAD;                   // 26: where the adjoint needs D1, D2, D3
constexpr int RING = MID * MID - LT * LT;           // 420 pixels of that square outside the tile
constexpr int LOSS_THREADS = LT * LT;

struct SsimTerms { double S, D1, D2, D3; };

// The pointwise part of the contract from the five filtered moments (mu1, mu2, m_aa, m_bb, m_ab).  S is formed exactly as
// k_metrics_tiles forms it.
__device__ __forceinline__ SsimTerms ssim_terms(const double (&m)[5]) {
    const double mu1 = m[0], mu2 = m[1], mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
    const double A1 = 2.0 * mu12 + SSIM_C1, A2 = 2.0 * s12 + SSIM_C2, B1 = (mu1_sq + mu2_sq) + SSIM_C1, B2 = (s1 + s2) + SSIM_C2;
    const double P = B1 * B2, inv = 1.0 / P, rB1 = 1.0 / B1, rB2 = 1.0 / B2;
    SsimTerms r;
    r.S = (A1 * A2) / P;
    const double tm2 = 2.0 * mu2, tm1S = (2.0 * mu1) * r.S;
    r.D1 = (((tm2 * A2) * inv - (tm2 * A1) * inv) - tm1S * rB1) + tm1S * rB2;
    r.D2 = -(r.S * rB2);
    r.D3 = (2.0 * A1) * inv;
    return r;
}

template <bool GRAD>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_tiles(int32_t H, int32_t W, SsimWindow win, double c_l1, double c_ssim, const float* __restrict__ A,
                                                             const float* __restrict__ B, double* __restrict__ partials, float* __restrict__ grad) {
    constexpr int HALO = GRAD ? 2 * RAD : RAD;      // staged pixels around the tile
    constexpr int SIN = LT + 2 * HALO;              // 36 (26): the staged square
    constexpr int NQ = SIN - 2 * RAD;               // 26 (16): columns the horizontal pass leaves
    constexpr int OFF = HALO - RAD;                 // 5 (0): the tile's corner in the coordinates of the moments
    __shared__ float s_a[SIN][SIN + 1], s_b[SIN][SIN + 1];
    __shared__ double s_m[5 * SIN * NQ];            // [5][SIN][NQ] moment rows; from pass 4 on [3][MID][LT], the rows of D1, D2, D3
    __shared__ double s_d[GRAD ? 3 * MID * MID : 1];
    const int t = threadIdx.x, lx = t & (LT - 1), ly = t >> 4;
    const int x0 = blockIdx.x * LT, y0 = blockIdx.y * LT;
    const bool own = x0 + lx < W && y0 + ly < H;
    double acc[2] = {0.0, 0.0};                     // sum |a - b|, sum S over this thread's pixel
    for (int ch = 0; ch < 3; ++ch) {
        // 1. stage
        for (int k = t; k < SIN * SIN; k += LOSS_THREADS) {
            const int r = k / SIN, q = k - r * SIN;
            const int y = y0 + r - HALO, x = x0 + q - HALO;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            const int64_t at = ((int64_t)y * W + x) * 3 + ch;
            s_a[r][q] = in ? A[at] : 0.0f;
            s_b[r][q] = in ? B[at] : 0.0f;
        }
        __syncthreads();
        // 2. horizontal moments
        for (int k = t; k < SIN * NQ; k += LOSS_THREADS) {
            const int r = k / NQ, q = k - r * NQ;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
#pragma unroll
            for (int j = 0; j < SSIM_WIN; ++j) {
                const double a = (double)s_a[r][q + j], b = (double)s_b[r][q + j], w = win.w[j];
                m0 += w * a; m1 += w * b; m2 += w * (a * a); m3 += w * (b * b); m4 += w * (a * b);
            }
            s_m[k] = m0; s_m[SIN * NQ + k] = m1; s_m[2 * SIN * NQ + k] = m2; s_m[3 * SIN * NQ + k] = m3; s_m[4 * SIN * NQ + k] = m4;
        }
        __syncthreads();
        // 3. vertical moments and the pointwise terms: (r, q) in the coordinates of the tile +- 5 with the gradient, of the tile without
        auto terms_at = [&](int r, int q) {
            double m[5] = {0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < SSIM_WIN; ++j)
#pragma unroll
                for (int i = 0; i < 5; ++i) m[i] += win.w[j] * s_m[(i * SIN + r + j) * NQ + q];
            return ssim_terms(m);
        };
        {
            const SsimTerms T = terms_at(ly + OFF, lx + OFF);
            if (own) acc[1] += T.S;
            if constexpr (GRAD) {
                const int at = (ly + RAD) * MID + lx + RAD;
                s_d[at] = own ? T.D1 : 0.0; s_d[MID * MID + at] = own ? T.D2 : 0.0; s_d[2 * MID * MID + at] = own ? T.D3 : 0.0;
            }
        }
        if constexpr (GRAD) {
            for (int e = t; e < RING; e += LOSS_THREADS) {
                int r, q;
                if (e < 2 * RAD * MID) {                        // the five rows above the tile, then the five below
                    r = e / MID; q = e - r * MID;
                    if (r >= RAD) r += LT;
                } else {                                        // the five columns left of it and the five right of it, row by row
                    const int f = e - 2 * RAD * MID;
                    r = f / (2 * RAD); q = f - r * (2 * RAD);
                    r += RAD;
                    if (q >= RAD) q += LT;
                }
                const int y = y0 + r - RAD, x = x0 + q - RAD;
                const bool in = y >= 0 && y < H && x >= 0 && x < W;
                const SsimTerms T = terms_at(r, q);
                const int at = r * MID + q;
                s_d[at] = in ? T.D1 : 0.0; s_d[MID * MID + at] = in ? T.D2 : 0.0; s_d[2 * MID * MID + at] = in ? T.D3 : 0.0;
            }
            __syncthreads();
            // 4. horizontal pass over the three maps
            for (int k = t; k < MID * LT; k += LOSS_THREADS) {
                const int r = k / LT, q = k - r * LT;
                double h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
                for (int j = 0; j < SSIM_WIN; ++j) {
                    const double w = win.w[j];
                    h0 += w * s_d[r * MID + q + j]; h1 += w * s_d[MID * MID + r * MID + q + j]; h2 += w * s_d[2 * MID * MID + r * MID + q + j];
                }
                s_m[k] = h0; s_m[MID * LT + k] = h1; s_m[2 * MID * LT + k] = h2;
            }
            __syncthreads();
        }
        // 5. the L1 term of the own pixel; with the gradient the vertical pass, the combination and the store
        const float af = s_a[ly + HALO][lx + HALO], bf = s_b[ly + HALO][lx + HALO];
        const double a = (double)af, b = (double)bf, d = a - b;
        if (own) acc[0] += fabs(d);
        if constexpr (GRAD) {
            double g0 = 0, g1 = 0, g2 = 0;
#pragma unroll
            for (int j = 0; j < SSIM_WIN; ++j) {
                const double w = win.w[j];
                const int at = (ly + j) * LT + lx;
                g0 += w * s_m[at]; g1 += w * s_m[MID * LT + at]; g2 += w * s_m[2 * MID * LT + at];
            }
            if (own) {
                const double sgn = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
                const double conv = (g0 + (2.0 * a) * g1) + b * g2;
                grad[((int64_t)(y0 + ly) * W + (x0 + lx)) * 3 + ch] = (float)(c_l1 * sgn - c_ssim * conv);
            }
        }
        __syncthreads();                            // the next channel overwrites s_a, s_b and s_m
    }
    block_fold_store<2, 2, wave_sum_xor>(acc, partials, (int)(blockIdx.y * gridDim.x + blockIdx.x));
}

// out = (loss, l1, ssim) from the two folded sums
__global__ void k_loss_outputs(double count, double lambda, const double* __restrict__ sums, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double l1 = sums[0] / count, ssim = sums[1] / count;
    out[0] = (1.0 - lambda) * l1 + lambda * (1.0 - ssim);
    out[1] = l1;
    out[2] = ssim;
}

}  // namespace

struct gsr_loss_ctx {
    int device = 0;
    DevBuf partials;        // two float64 per tile, grow-only
    DevBuf sums;            // the two folded sums
    ~gsr_loss_ctx() { (void)hipSetDevice(device); }      // (the members' hipFree waits for the work that still reads them)
};

extern "C" int32_t gsr_loss_create(int32_t device, gsr_loss_ctx** out) {
    if (!out) return fail(GSR_E_INVALID, "gsr_loss_create: out is NULL");
    *out = nullptr;
    GSR_TRY(open_device(device, "gsr_loss_create"));
    gsr_loss_ctx* c = new gsr_loss_ctx();
    c->device = device;
    const int32_t r = c->sums.reserve(2 * sizeof(double));
    if (r != GSR_OK) { delete c; return r; }
    *out = c;
    return GSR_OK;
}

extern "C" int32_t gsr_loss_destroy(gsr_loss_ctx* c) {
    delete c;       // (NULL: nothing)
    return GSR_OK;
}

extern "C" int32_t gsr_loss_l1_dssim(gsr_loss_ctx* c, const float* image, const float* target, int32_t height, int32_t width, double lambda,
                                     double* loss_out, float* grad_image, void* stream) {
    if (!c || !image || !target || !loss_out) return fail(GSR_E_INVALID, "gsr_loss_l1_dssim: NULL argument");
    if (height <= 0 || width <= 0) return fail(GSR_E_INVALID, "gsr_loss_l1_dssim: image size %d x %d", height, width);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(GSR_E_INVALID, "gsr_loss_l1_dssim: lambda %g outside [0, 1]", lambda);
    const dim3 grid((width + LT - 1) / LT, (height + LT - 1) / LT);
    if (grid.y > 65535u) return fail(GSR_E_INVALID, "gsr_loss_l1_dssim: image too tall");
    const int64_t tiles = (int64_t)grid.x * grid.y;
    if (tiles > INT32_MAX) return fail(GSR_E_INVALID, "gsr_loss_l1_dssim: image too large");
    GSR_TRY(open_device(c->device, "gsr_loss_l1_dssim"));
    GSR_TRY(c->partials.reserve((size_t)tiles * 2 * sizeof(double)));
    const SsimWindow win = ssim_window();
    const double count = 3.0 * (double)height * (double)width;
    const double c_l1 = (1.0 - lambda) / count, c_ssim = lambda / count;
    hipStream_t st = (hipStream_t)stream;
    double *partials = c->partials.as<double>(), *sums = c->sums.as<double>();
    if (grad_image)
        hipLaunchKernelGGL(k_loss_tiles<true>, grid, dim3(LOSS_THREADS), 0, st, height, width, win, c_l1, c_ssim, image, target, partials, grad_image);
    else
        hipLaunchKernelGGL(k_loss_tiles<false>, grid, dim3(LOSS_THREADS), 0, st, height, width, win, c_l1, c_ssim, image, target, partials, (float*)nullptr);
    hipLaunchKernelGGL(k_fold_partials<256>, dim3(2), dim3(256), 0, st, tiles, 2, (const double*)partials, sums);
    hipLaunchKernelGGL(k_loss_outputs, dim3(1), dim3(64), 0, st, count, lambda, (const double*)sums, loss_out);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}
