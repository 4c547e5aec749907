// photo.hip -- the sums of render-based photometric refinement (gsr_photo_accumulate; include/gsr_hip.h).
// The definition is restated in float64 in tests/photo_model.py; the loop around it is Python (photo.py).
//
//   k_photo_tiles     a group per 16 x 16 tile, a lane per pixel.  The tile's target intensity (float64), depth and coverage with a
//                     one-pixel halo go to LDS (zeros outside the image) for the Sobel taps and the nine-pixel coverage test; every
//                     lane forms its two Jacobian rows and residuals in float64 (14 values), and each of the 30 terms is folded as
//                     it is formed, in the fixed order of gsr_fold.h (the xor tree per wave, the four waves in order).  No per-lane
//                     array of 30 accumulators lives across the fold.
//   k_fold_partials<256>  one group of 256 per sum adds the groups' partials (gsr_fold.h).
// No atomics: the same inputs give the same bits.
#include "gsr_common.h"
#include "gsr_fold.h"
#include "gsr_oneshot.h"

#include <float.h>
#include <math.h>
#include <string.h>

namespace gsr {

constexpr int PT = 16, PTH = PT + 2;          // 16 x 16 pixels per group, 18 x 18 with the halo

struct PhotoCam {
    double R[9], t[3];                        // world -> camera, row-major
    double fx, fy, cx, cy;
    double sI, sD;                            // sqrt(1 - lambda), sqrt(lambda)
    double tau, max_dd;
};

__global__ __launch_bounds__(PT * PT) void k_photo_tiles(int32_t H, int32_t W, PhotoCam cam, const float* __restrict__ Is, const float* __restrict__ Ds,
                                                         const float* __restrict__ As, const float* __restrict__ It, const float* __restrict__ Dt,
                                                         const float* __restrict__ At, double* __restrict__ partial) {
    __shared__ double s_y[PTH][PTH + 1];
    __shared__ float s_d[PTH][PTH + 1], s_a[PTH][PTH + 1];
    __shared__ double s_red[4][GSR_PHOTO_SUMS_LEN];
    const int t = threadIdx.x, lx = t & (PT - 1), ly = t >> 4;
    const int x0 = blockIdx.x * PT, y0 = blockIdx.y * PT;
    for (int k = t; k < PTH * PTH; k += PT * PT) {
        const int r = k / PTH, q = k - r * PTH;
        const int y = y0 + r - 1, x = x0 + q - 1;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const int64_t pix = in ? (int64_t)y * W + x : 0;
        const double cr = in ? (double)It[3 * pix] : 0.0, cg = in ? (double)It[3 * pix + 1] : 0.0, cb = in ? (double)It[3 * pix + 2] : 0.0;
        s_y[r][q] = (0.299 * cr + 0.587 * cg) + 0.114 * cb;
        s_d[r][q] = in ? Dt[pix] : 0.0f;
        s_a[r][q] = in ? At[pix] : 0.0f;          // outside the image: coverage 0 < tau, the nine-pixel test fails
    }
    __syncthreads();
    const int x = x0 + lx, y = y0 + ly;
    bool ok = false;
    double JI[6] = {0, 0, 0, 0, 0, 0}, JD[6] = {0, 0, 0, 0, 0, 0}, rI = 0.0, rD = 0.0;
    if (x < W && y < H) {
        const int64_t pix = (int64_t)y * W + x;
        const double as = (double)As[pix], z = (double)Ds[pix], dt = (double)s_d[ly + 1][lx + 1];
        bool nine = true;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) nine = nine && (double)s_a[ly + dy][lx + dx] >= cam.tau;
        ok = nine && as >= cam.tau && fabs(dt - z) <= cam.max_dd;
        if (ok) {
            const double sr = (double)Is[3 * pix], sg = (double)Is[3 * pix + 1], sb = (double)Is[3 * pix + 2];
            const double ys = (0.299 * sr + 0.587 * sg) + 0.114 * sb;
            const double u = (double)x + 0.5, v = (double)y + 0.5;
            const double xn = (u - cam.cx) / cam.fx, yn = (v - cam.cy) / cam.fy;
            const double X = z * xn, Y = z * yn;
            const double q0 = X - cam.t[0], q1 = Y - cam.t[1], q2 = z - cam.t[2];
            double pw[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) pw[i] = (cam.R[i] * q0 + cam.R[3 + i] * q1) + cam.R[6 + i] * q2;
            double M[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double r0 = cam.R[3 * r], r1 = cam.R[3 * r + 1], r2 = cam.R[3 * r + 2];
                M[r][0] = r2 * pw[1] - r1 * pw[2];
                M[r][1] = r0 * pw[2] - r2 * pw[0];
                M[r][2] = r1 * pw[0] - r0 * pw[1];
                M[r][3] = r0; M[r][4] = r1; M[r][5] = r2;
            }
            // Sobel over 8 of the target maps: the taps of LDS rows ly .. ly + 2, columns lx .. lx + 2
#define PHOTO_SOBEL_X(F) (((((double)F[ly][lx + 2] - (double)F[ly][lx]) + 2.0 * ((double)F[ly + 1][lx + 2] - (double)F[ly + 1][lx])) + \
                           ((double)F[ly + 2][lx + 2] - (double)F[ly + 2][lx])) * 0.125)
#define PHOTO_SOBEL_Y(F) (((((double)F[ly + 2][lx] - (double)F[ly][lx]) + 2.0 * ((double)F[ly + 2][lx + 1] - (double)F[ly][lx + 1])) + \
                           ((double)F[ly + 2][lx + 2] - (double)F[ly][lx + 2])) * 0.125)
            const double gYx = PHOTO_SOBEL_X(s_y), gYy = PHOTO_SOBEL_Y(s_y), gDx = PHOTO_SOBEL_X(s_d), gDy = PHOTO_SOBEL_Y(s_d);
#undef PHOTO_SOBEL_X
#undef PHOTO_SOBEL_Y
            const double a0 = (gYx * cam.fx) / z, a1 = (gYy * cam.fy) / z, a2 = -((a0 * X + a1 * Y) / z);
            const double d0 = (gDx * cam.fx) / z, d1 = (gDy * cam.fy) / z, d2 = -((d0 * X + d1 * Y) / z) - 1.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                JI[k] = cam.sI * ((a0 * M[0][k] + a1 * M[1][k]) + a2 * M[2][k]);
                JD[k] = cam.sD * ((d0 * M[0][k] + d1 * M[1][k]) + d2 * M[2][k]);
            }
            rI = cam.sI * (s_y[ly + 1][lx + 1] - ys);
            rD = cam.sD * (dt - z);
        }
    }
    // the group's fold (block_fold_store's, gsr_fold.h), one term at a time.  A pixel that does not count adds +0.0.
    const int lane = t & 63, wv = t >> 6;
    const bool any = __any(ok) != 0;                 // a wave without a counted pixel: thirty zeros, no tree
#define PHOTO_FOLD(K, TERM)                                                        \
    {                                                                              \
        const double v_ = any ? wave_sum_xor(TERM) : 0.0;                          \
        if (lane == 0) s_red[wv][K] = v_;                                          \
    }
    {
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { PHOTO_FOLD(k, JI[r] * JI[c] + JD[r] * JD[c]); ++k; }
#pragma unroll
        for (int r = 0; r < 6; ++r) { PHOTO_FOLD(21 + r, JI[r] * rI + JD[r] * rD); }
        PHOTO_FOLD(27, rI * rI);
        PHOTO_FOLD(28, rD * rD);
        PHOTO_FOLD(29, ok ? 1.0 : 0.0);
    }
#undef PHOTO_FOLD
    __syncthreads();
    if (t < GSR_PHOTO_SUMS_LEN) {
        const int64_t g = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[g * GSR_PHOTO_SUMS_LEN + t] = ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t];
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_photo_accumulate(const float* I_s, const float* D_s, const float* A_s, const float* I_t, const float* D_t, const float* A_t,
                                        int32_t height, int32_t width, const double* viewmat16, double fx, double fy, double cx, double cy, double lambda,
                                        double tau, double max_depth_diff, int32_t on_device, double* out30, int32_t device, void* stream) {
    const char* who = "gsr_photo_accumulate";
    auto finite = [](double v) { return fabs(v) <= DBL_MAX; };
    if (!I_s || !D_s || !A_s || !I_t || !D_t || !A_t || !viewmat16 || !out30) return fail(GSR_E_INVALID, "gsr_photo_accumulate: NULL argument");
    if (height <= 0 || width <= 0) return fail(GSR_E_INVALID, "gsr_photo_accumulate: image size %d x %d must be positive", width, height);
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(GSR_E_INVALID, "gsr_photo_accumulate: lambda must be in [0, 1]");
    if (!(tau > 0.0 && tau <= 1.0)) return fail(GSR_E_INVALID, "gsr_photo_accumulate: tau must be in (0, 1]");
    if (!(max_depth_diff > 0.0) || !finite(max_depth_diff)) return fail(GSR_E_INVALID, "gsr_photo_accumulate: max_depth_diff must be positive and finite");
    for (int k = 0; k < 16; ++k)
        if (!finite(viewmat16[k])) return fail(GSR_E_INVALID, "gsr_photo_accumulate: the camera is not finite (viewmat[%d])", k);
    if (!finite(fx) || !finite(fy) || !finite(cx) || !finite(cy)) return fail(GSR_E_INVALID, "gsr_photo_accumulate: the camera is not finite (intrinsics)");
    if (!(fx > 0.0) || !(fy > 0.0)) return fail(GSR_E_INVALID, "gsr_photo_accumulate: focal lengths must be positive");
    const dim3 grid((width + PT - 1) / PT, (height + PT - 1) / PT);
    if (grid.y > 65535u) return fail(GSR_E_INVALID, "gsr_photo_accumulate: image too tall");
    GSR_TRY(open_device(device, who));
    PhotoCam cam;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) cam.R[3 * r + c] = viewmat16[4 * r + c];
        cam.t[r] = viewmat16[4 * r + 3];
    }
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    cam.sI = sqrt(1.0 - lambda); cam.sD = sqrt(lambda);
    cam.tau = tau; cam.max_dd = max_depth_diff;
    const size_t npix = (size_t)height * (size_t)width;
    const int64_t groups = (int64_t)grid.x * grid.y;
    double host[GSR_PHOTO_SUMS_LEN];
    {
        OneShot os((hipStream_t)stream, on_device != 0, who);
        const float *dIs, *dDs, *dAs, *dIt, *dDt, *dAt;
        double *partial = nullptr, *res = nullptr;
        GSR_TRY(os.in(I_s, npix * 12, &dIs));
        GSR_TRY(os.in(D_s, npix * 4, &dDs));
        GSR_TRY(os.in(A_s, npix * 4, &dAs));
        GSR_TRY(os.in(I_t, npix * 12, &dIt));
        GSR_TRY(os.in(D_t, npix * 4, &dDt));
        GSR_TRY(os.in(A_t, npix * 4, &dAt));
        GSR_TRY(os.scratch((size_t)groups * GSR_PHOTO_SUMS_LEN * sizeof(double), &partial));
        GSR_TRY(os.scratch(GSR_PHOTO_SUMS_LEN * sizeof(double), &res));
        hipLaunchKernelGGL(k_photo_tiles, grid, dim3(PT * PT), 0, os.st, height, width, cam, dIs, dDs, dAs, dIt, dDt, dAt, partial);
        hipLaunchKernelGGL(k_fold_partials<256>, dim3(GSR_PHOTO_SUMS_LEN), dim3(256), 0, os.st, groups, GSR_PHOTO_SUMS_LEN, (const double*)partial, res);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, os.st);
        GSR_TRY(os.wait(e));
    }
    memcpy(out30, host, sizeof(host));
    return GSR_OK;
}
