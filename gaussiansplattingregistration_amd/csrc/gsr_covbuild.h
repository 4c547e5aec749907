// gsr_covbuild.h -- (log-scale, raw quaternion) -> covariance, and its derivative, written once.
//
// Forward (float32, what 3DGS's build_rotation / build_scaling_rotation / strip_symmetric compute, general_utils.py:43-80): with a row's
// log-scales s and raw quaternion q = (w, x, y, z),
//     n = |q|,  u = q / n,  e = exp(s),  L = R(u) diag(e),  cov = L L^T   (xx, xy, xz, yy, yz, zz).
// k_ply_unpack (csrc/model.hip) and k_cov_build (csrc/covgrad.hip) both call cov_build, so the loader's covariance and a rebuilt one
// have the same bits; the library is compiled with -ffp-contract=off, and every sum here is associated as (a + b) + c.
//
// Backward: g6 = dLoss / dcov6 in the convention of gsr_raster_backward -- an off-diagonal entry of cov6 stands for both symmetric
// positions.  G is the symmetric 3x3 with G_ii = g6_ii and G_ij = g6_ij / 2, so dLoss = sum_ij G_ij dcov_ij, and
//     M = 2 G L,   dLoss/ds_k = e_k sum_i M_ik R_ik,   D_ik = M_ik e_k = dLoss/dR_ik,
//     dLoss/du = D contracted with dR/du,   dLoss/dq = (dLoss/du - u (u . dLoss/du)) / n.
// The function does not depend on |q|: q . dLoss/dq = 0 up to rounding, and dLoss/dq scales with 1 / |q|.
// cov_build_backward recomputes u, e, R and L through cov_factors, the function the forward uses: the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace gsr {

struct CovFactors {
    float nrm;                  // |q|
    float w, x, y, z;           // u = q / |q|
    float e0, e1, e2;           // exp(s)
    float R00, R01, R02, R10, R11, R12, R20, R21, R22;
    float l00, l01, l02, l10, l11, l12, l20, l21, l22;          // L = R diag(e)
};

__device__ __forceinline__ CovFactors cov_factors(float s0, float s1, float s2, float qw, float qx, float qy, float qz) {
    CovFactors F;
    F.nrm = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    const float w = qw / F.nrm, x = qx / F.nrm, y = qy / F.nrm, z = qz / F.nrm;
    F.w = w; F.x = x; F.y = y; F.z = z;
    F.e0 = expf(s0); F.e1 = expf(s1); F.e2 = expf(s2);
    F.R00 = 1.0f - 2.0f * (y * y + z * z); F.R01 = 2.0f * (x * y - w * z); F.R02 = 2.0f * (x * z + w * y);
    F.R10 = 2.0f * (x * y + w * z); F.R11 = 1.0f - 2.0f * (x * x + z * z); F.R12 = 2.0f * (y * z - w * x);
    F.R20 = 2.0f * (x * z - w * y); F.R21 = 2.0f * (y * z + w * x); F.R22 = 1.0f - 2.0f * (x * x + y * y);
    F.l00 = F.R00 * F.e0; F.l01 = F.R01 * F.e1; F.l02 = F.R02 * F.e2;
    F.l10 = F.R10 * F.e0; F.l11 = F.R11 * F.e1; F.l12 = F.R12 * F.e2;
    F.l20 = F.R20 * F.e0; F.l21 = F.R21 * F.e1; F.l22 = F.R22 * F.e2;
    return F;
}

// cov[6] = (xx, xy, xz, yy, yz, zz) of L L^T
__device__ __forceinline__ void cov_build(float s0, float s1, float s2, float qw, float qx, float qy, float qz, float cov[6]) {
    const CovFactors F = cov_factors(s0, s1, s2, qw, qx, qy, qz);
    cov[0] = (F.l00 * F.l00 + F.l01 * F.l01) + F.l02 * F.l02; cov[1] = (F.l00 * F.l10 + F.l01 * F.l11) + F.l02 * F.l12;
    cov[2] = (F.l00 * F.l20 + F.l01 * F.l21) + F.l02 * F.l22; cov[3] = (F.l10 * F.l10 + F.l11 * F.l11) + F.l12 * F.l12;
    cov[4] = (F.l10 * F.l20 + F.l11 * F.l21) + F.l12 * F.l22; cov[5] = (F.l20 * F.l20 + F.l21 * F.l21) + F.l22 * F.l22;
}

// g[6] = dLoss/dcov6 -> gs[3] = dLoss/ds, gq[4] = dLoss/dq (w, x, y, z).  A row whose six g are all zero gets +0.0 in both, whatever its
// scale and quaternion (0 * exp(100) would be NaN); every other row gets what the arithmetic gives.
__device__ __forceinline__ void cov_build_backward(float s0, float s1, float s2, float qw, float qx, float qy, float qz, const float g[6], float gs[3],
                                                   float gq[4]) {
    if (g[0] == 0.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f && g[4] == 0.0f && g[5] == 0.0f) {
        gs[0] = gs[1] = gs[2] = 0.0f;
        gq[0] = gq[1] = gq[2] = gq[3] = 0.0f;
        return;
    }
    const CovFactors F = cov_factors(s0, s1, s2, qw, qx, qy, qz);
    const float G00 = g[0], G01 = 0.5f * g[1], G02 = 0.5f * g[2], G11 = g[3], G12 = 0.5f * g[4], G22 = g[5];
    // M = 2 G L
    const float M00 = 2.0f * ((G00 * F.l00 + G01 * F.l10) + G02 * F.l20), M01 = 2.0f * ((G00 * F.l01 + G01 * F.l11) + G02 * F.l21),
                M02 = 2.0f * ((G00 * F.l02 + G01 * F.l12) + G02 * F.l22);
    const float M10 = 2.0f * ((G01 * F.l00 + G11 * F.l10) + G12 * F.l20), M11 = 2.0f * ((G01 * F.l01 + G11 * F.l11) + G12 * F.l21),
                M12 = 2.0f * ((G01 * F.l02 + G11 * F.l12) + G12 * F.l22);
    const float M20 = 2.0f * ((G02 * F.l00 + G12 * F.l10) + G22 * F.l20), M21 = 2.0f * ((G02 * F.l01 + G12 * F.l11) + G22 * F.l21),
                M22 = 2.0f * ((G02 * F.l02 + G12 * F.l12) + G22 * F.l22);
    gs[0] = F.e0 * ((M00 * F.R00 + M10 * F.R10) + M20 * F.R20);
    gs[1] = F.e1 * ((M01 * F.R01 + M11 * F.R11) + M21 * F.R21);
    gs[2] = F.e2 * ((M02 * F.R02 + M12 * F.R12) + M22 * F.R22);
    // D = M diag(e) = dLoss/dR
    const float D00 = M00 * F.e0, D01 = M01 * F.e1, D02 = M02 * F.e2, D10 = M10 * F.e0, D11 = M11 * F.e1, D12 = M12 * F.e2, D20 = M20 * F.e0, D21 = M21 * F.e1,
                D22 = M22 * F.e2;
    const float w = F.w, x = F.x, y = F.y, z = F.z;
    // dLoss/du: D contracted with the derivative of R(u)
    const float uw = 2.0f * ((x * (D21 - D12) + y * (D02 - D20)) + z * (D10 - D01));
    const float ux = 2.0f * (((y * (D01 + D10) + z * (D02 + D20)) + w * (D21 - D12)) - (2.0f * x) * (D11 + D22));
    const float uy = 2.0f * (((x * (D01 + D10) + z * (D12 + D21)) + w * (D02 - D20)) - (2.0f * y) * (D00 + D22));
    const float uz = 2.0f * (((x * (D02 + D20) + y * (D12 + D21)) + w * (D10 - D01)) - (2.0f * z) * (D00 + D11));
    // through u = q / |q|: the component along u drops out
    const float dot = ((w * uw + x * ux) + y * uy) + z * uz;
    gq[0] = (uw - w * dot) / F.nrm; gq[1] = (ux - x * dot) / F.nrm; gq[2] = (uy - y * dot) / F.nrm; gq[3] = (uz - z * dot) / F.nrm;
}

}  // namespace gsr
