// covgrad.hip -- covariance of every splat from its log-scales and raw quaternion, and the derivative of that map: gsr_cov_build and
// gsr_cov_build_backward (include/gsr_hip.h).  The arithmetic is gsr_covbuild.h's, the one k_ply_unpack (csrc/model.hip)
// runs on the rows of a .ply: a covariance rebuilt here has the loader's bits.
//
// Both kernels stream: one thread per splat, grid-stride, no shared memory, no atomics -- the same inputs give the same bits.  The AoS
// rows (3, 4 and 6 floats) are read entry by entry as k_decompose_cov and k_ply_unpack read and write them: neighbouring lanes hold
// neighbouring rows, so the loads of a wave cover one contiguous span of 768, 1 024 or 1 536 bytes and every cache line fetched is used
// in full.  The backward recomputes u, e, R and L (cov_factors) instead of reading them: 52 bytes in, 28 bytes out per splat.
#include "gsr_common.h"
#include "gsr_covbuild.h"
#include "gsr_oneshot.h"

namespace gsr {

__global__ __launch_bounds__(256) void k_cov_build(int64_t n, const float* __restrict__ scaling, const float* __restrict__ rotation, float* __restrict__ cov6) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
        const float qw = rotation[4 * i], qx = rotation[4 * i + 1], qy = rotation[4 * i + 2], qz = rotation[4 * i + 3];
        float c[6];
        cov_build(s0, s1, s2, qw, qx, qy, qz, c);
        cov6[6 * i] = c[0]; cov6[6 * i + 1] = c[1]; cov6[6 * i + 2] = c[2]; cov6[6 * i + 3] = c[3]; cov6[6 * i + 4] = c[4]; cov6[6 * i + 5] = c[5];
    }
}

// grad_scaling / grad_rotation: either may be NULL (uniform over the grid) and is then not written
__global__ __launch_bounds__(256) void k_cov_build_backward(int64_t n, const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                            const float* __restrict__ grad_cov6, float* __restrict__ grad_scaling,
                                                            float* __restrict__ grad_rotation) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
        const float qw = rotation[4 * i], qx = rotation[4 * i + 1], qy = rotation[4 * i + 2], qz = rotation[4 * i + 3];
        const float g[6] = {grad_cov6[6 * i], grad_cov6[6 * i + 1], grad_cov6[6 * i + 2], grad_cov6[6 * i + 3], grad_cov6[6 * i + 4], grad_cov6[6 * i + 5]};
        float gs[3], gq[4];
        cov_build_backward(s0, s1, s2, qw, qx, qy, qz, g, gs, gq);
        if (grad_scaling) { grad_scaling[3 * i] = gs[0]; grad_scaling[3 * i + 1] = gs[1]; grad_scaling[3 * i + 2] = gs[2]; }
        if (grad_rotation) { grad_rotation[4 * i] = gq[0]; grad_rotation[4 * i + 1] = gq[1]; grad_rotation[4 * i + 2] = gq[2]; grad_rotation[4 * i + 3] = gq[3]; }
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_cov_build(const float* scaling, const float* rotation, int64_t n, float* cov6, int32_t on_device, int32_t device, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID, "gsr_cov_build: n = %lld is negative", (long long)n);
    if (n > 0 && (!scaling || !rotation || !cov6))
        return fail(GSR_E_INVALID, "gsr_cov_build: %s is NULL", !scaling ? "scaling" : (!rotation ? "rotation" : "cov6"));
    GSR_TRY(open_device(device, "gsr_cov_build"));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_cov_build");
    const float *sc = nullptr, *q = nullptr;
    float* c = nullptr;
    GSR_TRY(os.in(scaling, (size_t)n * 12, &sc));
    GSR_TRY(os.in(rotation, (size_t)n * 16, &q));
    GSR_TRY(os.out(cov6, (size_t)n * 24, &c));
    hipLaunchKernelGGL(k_cov_build, dim3(stride_grid(n)), dim3(256), 0, os.st, n, sc, q, c);
    return os.finish();
}

extern "C" int32_t gsr_cov_build_backward(const float* scaling, const float* rotation, const float* grad_cov6, int64_t n, float* grad_scaling,
                                          float* grad_rotation, int32_t on_device, int32_t device, void* stream) {
    if (n < 0) return fail(GSR_E_INVALID, "gsr_cov_build_backward: n = %lld is negative", (long long)n);
    if (n > 0 && (!scaling || !rotation || !grad_cov6))
        return fail(GSR_E_INVALID, "gsr_cov_build_backward: %s is NULL", !scaling ? "scaling" : (!rotation ? "rotation" : "grad_cov6"));
    if (n > 0 && !grad_scaling && !grad_rotation) return fail(GSR_E_INVALID, "gsr_cov_build_backward: grad_scaling and grad_rotation are both NULL");
    GSR_TRY(open_device(device, "gsr_cov_build_backward"));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_cov_build_backward");
    const float *sc = nullptr, *q = nullptr, *g = nullptr;
    float *gs = nullptr, *gq = nullptr;
    GSR_TRY(os.in(scaling, (size_t)n * 12, &sc));
    GSR_TRY(os.in(rotation, (size_t)n * 16, &q));
    GSR_TRY(os.in(grad_cov6, (size_t)n * 24, &g));
    GSR_TRY(os.out(grad_scaling, (size_t)n * 12, &gs));
    GSR_TRY(os.out(grad_rotation, (size_t)n * 16, &gq));
    hipLaunchKernelGGL(k_cov_build_backward, dim3(stride_grid(n)), dim3(256), 0, os.st, n, sc, q, g, gs, gq);
    return os.finish();
}
