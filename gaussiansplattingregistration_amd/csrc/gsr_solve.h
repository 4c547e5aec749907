// gsr_solve.h -- float64 solves shared by csrc/icp.hip (the ICP estimators), csrc/features.hip (the RANSAC hypotheses), csrc/d2d.hip
// and csrc/fgr.hip (their 6-DoF steps): 3x3 Jacobi SVD (Eigen::umeyama), 6x6 LDL^T (Eigen's LDLT), the symmetric 6x6 from its 21
// upper-triangle sums, the rigid update of a 6-vector, and the estimator update from reduced accumulators.
#pragma once
#include "gsr_common.h"

#include <math.h>

namespace gsr {

// ---- float64 solves (host and device: the device-resident ICP loop runs them in one thread) ----------
__host__ __device__ static void svd3(const double Ain[3][3], double U[3][3], double s[3], double V[3][3]) {
    double B[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { B[i][j] = Ain[i][j]; V[i][j] = i == j; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; ++i) { alpha += B[i][p] * B[i][p]; beta += B[i][q] * B[i][q]; gamma += B[i][p] * B[i][q]; }
                if (gamma == 0) continue;
                off = fmax(off, fabs(gamma) / sqrt(alpha * beta + 1e-300));
                const double zeta = (beta - alpha) / (2 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1 + zeta * zeta));
                const double c = 1 / sqrt(1 + t * t), sn = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double bp = B[i][p], bq = B[i][q];
                    B[i][p] = c * bp - sn * bq; B[i][q] = sn * bp + c * bq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - sn * vq; V[i][q] = sn * vp + c * vq;
                }
            }
        if (off < 1e-17) break;
    }
    int order[3] = {0, 1, 2};
    double nrm[3];
    for (int j = 0; j < 3; ++j) nrm[j] = sqrt(B[0][j] * B[0][j] + B[1][j] * B[1][j] + B[2][j] * B[2][j]);
    for (int a = 0; a < 2; ++a) for (int b = a + 1; b < 3; ++b) if (nrm[order[b]] > nrm[order[a]]) { int t = order[a]; order[a] = order[b]; order[b] = t; }
    double Vs[3][3], Bs[3][3];
    for (int j = 0; j < 3; ++j) { s[j] = nrm[order[j]]; for (int i = 0; i < 3; ++i) { Vs[i][j] = V[i][order[j]]; Bs[i][j] = B[i][order[j]]; } }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = Vs[i][j];
    if (!(s[0] > 0)) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) U[i][j] = i == j; return; }
    for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) U[i][j] = s[j] > 0 ? Bs[i][j] / s[j] : 0.0;
    if (s[1] <= 1e-12 * s[0]) {
        double u0[3] = {U[0][0], U[1][0], U[2][0]};
        int k = fabs(u0[0]) < fabs(u0[1]) ? (fabs(u0[0]) < fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) < fabs(u0[2]) ? 1 : 2);
        double e[3] = {0, 0, 0};
        e[k] = 1;
        const double d = u0[k];
        double v[3] = {e[0] - d * u0[0], e[1] - d * u0[1], e[2] - d * u0[2]};
        const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int i = 0; i < 3; ++i) U[i][1] = v[i] / n;
    }
    if (s[2] <= 1e-12 * s[0]) {
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
}
__host__ __device__ static double det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
// x = A^-1 b by LDL^T with diagonal pivoting (what Eigen's LDLT, which Open3D's solvers call, does).  Every index below
// is a compile-time constant once the loops are unrolled -- the pivot's row / column exchange is a chain of tests against
// the constant candidates -- so on the device the 36 + 15 + 18 doubles live in registers: with run-time indices the
// arrays went to scratch memory (720 bytes per lane) and the single-thread solve of k_icp_step took ~15 us.
__host__ __device__ static void solve6(const double A_[6][6], const double b_[6], double x[6]) {
    double A[6][6], L[6][6], D[6], bp[6];
    int perm[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        perm[i] = i; bp[i] = b_[i];
#pragma unroll
        for (int j = 0; j < 6; ++j) { A[i][j] = A_[i][j]; L[i][j] = 0.0; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int piv = k;
        double best = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) { const double v = fabs(A[i][i]); if (v > best) { best = v; piv = i; } }
#pragma unroll
        for (int c = k + 1; c < 6; ++c) {
            if (piv == c) {
#pragma unroll
                for (int j = 0; j < 6; ++j) { const double t = A[k][j]; A[k][j] = A[c][j]; A[c][j] = t; }
#pragma unroll
                for (int i = 0; i < 6; ++i) { const double t = A[i][k]; A[i][k] = A[i][c]; A[i][c] = t; }
#pragma unroll
                for (int j = 0; j < k; ++j) { const double t = L[k][j]; L[k][j] = L[c][j]; L[c][j] = t; }
                const int t = perm[k]; perm[k] = perm[c]; perm[c] = t;
                const double tb = bp[k]; bp[k] = bp[c]; bp[c] = tb;        // bp[i] == b[perm[i]] throughout
            }
        }
        D[k] = A[k][k];
        L[k][k] = 1;
#pragma unroll
        for (int i = k + 1; i < 6; ++i) L[i][k] = A[i][k] / D[k];
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
#pragma unroll
            for (int j = k + 1; j < 6; ++j) A[i][j] -= L[i][k] * D[k] * L[j][k];
    }
    double y[6], z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = bp[i];
#pragma unroll
        for (int j = 0; j < i; ++j) s -= L[i][j] * y[j];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] /= D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) s -= L[j][i] * z[j];
        z[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c)
            if (perm[i] == c) x[c] = z[i];
}
__host__ __device__ static void mat4_identity(double T[16]) { for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0; }
__host__ __device__ static void mat4_mul(const double A[16], const double B[16], double C[16]) {
    double R[16];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j]; R[4 * i + j] = s; }
    for (int i = 0; i < 16; ++i) C[i] = R[i];
}
// A = the symmetric 6 x 6 whose upper triangle, row by row, is u21[0..20]
__host__ __device__ static inline void sym6_from_upper(const double* u21, double A[6][6]) {
    int t = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) { A[a][b] = u21[t]; A[b][a] = u21[t]; ++t; }
}
// M = the 4 x 4 (row-major) of the 6-DoF step x: rotation Rz(x2) Ry(x1) Rx(x0), translation x3..5
__host__ __device__ static inline void rigid_from_euler6(const double x[6], double M[16]) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    M[0] = cg * cb; M[1] = cg * sb * sa - sg * ca; M[2] = cg * sb * ca + sg * sa; M[3] = x[3];
    M[4] = sg * cb; M[5] = sg * sb * sa + cg * ca; M[6] = sg * sb * ca - cg * sa; M[7] = x[4];
    M[8] = -sb;     M[9] = cb * sa;                M[10] = cb * ca;               M[11] = x[5];
    M[12] = 0.0;    M[13] = 0.0;                   M[14] = 0.0;                   M[15] = 1.0;
}

// estimator update from the reduced accumulators (Open3D TransformationEstimation*.ComputeTransformation)
// GSR_ICP_POINT_TO_POINT_SCALED is Eigen::umeyama(src, dst, true): mp, mq, sigma, the SVD and the sign matrix S as for kind 0, then
//     var = acc[17] / n - |mp|^2,   c = (s0 S0 + s1 S1 + s2 S2) / var,   update = [c R | (mq + ctr) - c R (mp + ctr)].
// DEVIATION from Eigen: when !(var > 0) or !(c > 0) -- one correspondence, coincident sources, a rank-0 sigma -- Eigen divides by
// zero (a NaN / inf transform); here the update is the identity, as for no correspondences at all.
__host__ __device__ static void estimate_update(const double ctr[3], int kind, const double* acc, double update[16]) {
    mat4_identity(update);
    const double n = acc[0];
    if (!(n > 0)) return;                                   // no correspondences -> identity
    if (kind == GSR_ICP_POINT_TO_POINT || kind == GSR_ICP_POINT_TO_POINT_SCALED) {      // Eigen::umeyama(src, dst, with_scaling)
        const double mp[3] = {acc[2] / n, acc[3] / n, acc[4] / n}, mq[3] = {acc[5] / n, acc[6] / n, acc[7] / n};
        double sigma[3][3], U[3][3], V[3][3], s[3];
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 3; ++col) sigma[r][col] = acc[8 + 3 * col + r] / n - mq[r] * mp[col];   // dst x src^T
        svd3(sigma, U, s, V);
        double S[3] = {1, 1, 1};
        if (det3(U) * det3(V) < 0) S[2] = -1;
        double R[3][3];
        for (int r = 0; r < 3; ++r)
            for (int col = 0; col < 3; ++col) { double v = 0; for (int k = 0; k < 3; ++k) v += U[r][k] * S[k] * V[col][k]; R[r][col] = v; }
        if (kind == GSR_ICP_POINT_TO_POINT_SCALED) {
            const double var = acc[17] / n - (mp[0] * mp[0] + mp[1] * mp[1] + mp[2] * mp[2]);
            const double c = (s[0] * S[0] + s[1] * S[1] + s[2] * S[2]) / var;
            if (!(var > 0) || !(c > 0)) return;             // degenerate: the identity (see above)
            for (int r = 0; r < 3; ++r) for (int col = 0; col < 3; ++col) R[r][col] *= c;
        }
        for (int r = 0; r < 3; ++r) {
            for (int col = 0; col < 3; ++col) update[4 * r + col] = R[r][col];
            double Rp = 0;
            for (int col = 0; col < 3; ++col) Rp += R[r][col] * (mp[col] + ctr[col]);
            update[4 * r + 3] = mq[r] + ctr[r] - Rp;
        }
    } else {                                                 // x = solve(JTJ, -JTr)
        double JTJ[6][6], nb[6], x[6];
        sym6_from_upper(acc + 2, JTJ);
#pragma unroll
        for (int a = 0; a < 6; ++a) nb[a] = -acc[23 + a];
        solve6(JTJ, nb, x);
        rigid_from_euler6(x, update);
    }
}

}  // namespace gsr
