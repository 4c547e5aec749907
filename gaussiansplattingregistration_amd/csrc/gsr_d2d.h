// gsr_d2d.h -- mixture-to-mixture registration: the float64 math of ONE pair of components and of ONE source row,
// written once for the kernel (csrc/d2d.hip) and for the host (scripts/d2d_selftest.cpp compiles this file alone, with a host compiler and
// its sanitizers).  The definition is the header comment of include/gsr_hip.h; tests/d2d_model.py repeats every expression below in the
// same order.  Nothing here may be contracted into a fused multiply-add: the library is built with -ffp-contract=off.
// Needs nothing of HIP.  Not part of include/gsr_hip.h.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSR_D2D_HD __host__ __device__ __forceinline__
#else
#define GSR_D2D_HD inline
#endif

namespace gsr {
namespace d2d {

constexpr int SUMS_LEN = 32;      // GSR_D2D_SUMS_LEN
constexpr int S_SCORE = 27, S_WM = 28, S_PAIRS = 29, S_ROWS = 30, S_SINGULAR = 31;

GSR_D2D_HD bool finite(double x) { return x - x == 0.0; }

// p' = R p + t, a sum of products left to right; T = rows 0..2 of the 4 x 4, row-major
GSR_D2D_HD void move_point(const double* T, double x, double y, double z, double p[3]) {
    p[0] = T[0] * x + T[1] * y + T[2] * z + T[3];
    p[1] = T[4] * x + T[5] * y + T[6] * z + T[7];
    p[2] = T[8] * x + T[9] * y + T[10] * z + T[11];
}

// S = R A R' of a symmetric A (xx xy xz yy yz zz): first G = R A, G[a][b] = R[a][0] A[0][b] + R[a][1] A[1][b] + R[a][2] A[2][b], then
// S[a][b] = G[a][0] R[b][0] + G[a][1] R[b][1] + G[a][2] R[b][2] for a <= b
GSR_D2D_HD void rotate_cov(const double* T, const double A[6], double S[6]) {
    const double Af[3][3] = {{A[0], A[1], A[2]}, {A[1], A[3], A[4]}, {A[2], A[4], A[5]}};
    double G[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) G[a][b] = T[4 * a] * Af[0][b] + T[4 * a + 1] * Af[1][b] + T[4 * a + 2] * Af[2][b];
    int k = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) S[k++] = G[a][0] * T[4 * b] + G[a][1] * T[4 * b + 1] + G[a][2] * T[4 * b + 2];
}

// One pair.  S: the source's rotated covariance, B: the target's, s2 = cov_scale^2, phi = cov_floor, r = p' - q.
//   C_k = s2 (S_k + B_k), plus phi on the diagonal (k = 0, 3, 5)
//   adjugate: a0 = C3 C5 - C4 C4, a1 = C2 C4 - C1 C5, a2 = C1 C4 - C2 C3, a3 = C0 C5 - C2 C2, a4 = C1 C2 - C0 C4, a5 = C0 C3 - C1 C1
//   det = C0 a0 + C1 a1 + C2 a2; not (det > 0 and finite): singular, false is returned and nothing else is written
//   inv = 1 / det, M_k = a_k inv
//   Mr = (M0 r0 + M1 r1 + M2 r2, M1 r0 + M3 r1 + M4 r2, M2 r0 + M4 r1 + M5 r2), m = r0 Mr0 + r1 Mr1 + r2 Mr2
GSR_D2D_HD bool pair_metric(const double S[6], const double B[6], double s2, double phi, const double r[3], double M[6], double Mr[3], double* m) {
    const double C0 = s2 * (S[0] + B[0]) + phi, C1 = s2 * (S[1] + B[1]), C2 = s2 * (S[2] + B[2]);
    const double C3 = s2 * (S[3] + B[3]) + phi, C4 = s2 * (S[4] + B[4]), C5 = s2 * (S[5] + B[5]) + phi;
    const double a0 = C3 * C5 - C4 * C4, a1 = C2 * C4 - C1 * C5, a2 = C1 * C4 - C2 * C3;
    const double a3 = C0 * C5 - C2 * C2, a4 = C1 * C2 - C0 * C4, a5 = C0 * C3 - C1 * C1;
    const double det = C0 * a0 + C1 * a1 + C2 * a2;
    if (!(det > 0.0) || !finite(det)) return false;
    const double inv = 1.0 / det;
    M[0] = a0 * inv; M[1] = a1 * inv; M[2] = a2 * inv; M[3] = a3 * inv; M[4] = a4 * inv; M[5] = a5 * inv;
    Mr[0] = M[0] * r[0] + M[1] * r[1] + M[2] * r[2];
    Mr[1] = M[1] * r[0] + M[3] * r[1] + M[4] * r[2];
    Mr[2] = M[2] * r[0] + M[4] * r[1] + M[5] * r[2];
    *m = r[0] * Mr[0] + r[1] * Mr[1] + r[2] * Mr[2];
    return true;
}

// what a source row carries through its pairs, added in walk order: W = sum w M (six), b = sum w M r (three), sum w, sum w m, two counts
struct RowAcc {
    double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, s = 0.0, sm = 0.0;
    int pairs = 0, singular = 0;
};

// omega = (w v) exp(-m / 2) with the caller's exp; then the eleven additions
GSR_D2D_HD void row_add(RowAcc& a, double wv, double e, const double M[6], const double Mr[3], double m) {
    const double om = wv * e;
    for (int k = 0; k < 6; ++k) a.W[k] += om * M[k];
    for (int k = 0; k < 3; ++k) a.b[k] += om * Mr[k];
    a.s += om;
    a.sm += om * m;
    a.pairs += 1;
}

// The row's 32 values from its accumulators: J = [-[p']x | I3], so J' W J = [[P W P', P W], [., W]] and J' b = (P b, b) with
// P v = p' x v = (py vz - pz vy, pz vx - px vz, px vy - py vx).  A = P W column by column, H_rr row a = p' x (row a of A).
GSR_D2D_HD void row_expand(const double p[3], const RowAcc& a, double out[SUMS_LEN]) {
    const double* W = a.W;
    const double col[3][3] = {{W[0], W[1], W[2]}, {W[1], W[3], W[4]}, {W[2], W[4], W[5]}};
    double A[3][3], Hrr[3][3];
    for (int c = 0; c < 3; ++c) {
        A[0][c] = p[1] * col[c][2] - p[2] * col[c][1];
        A[1][c] = p[2] * col[c][0] - p[0] * col[c][2];
        A[2][c] = p[0] * col[c][1] - p[1] * col[c][0];
    }
    for (int r = 0; r < 3; ++r) {
        Hrr[r][0] = p[1] * A[r][2] - p[2] * A[r][1];
        Hrr[r][1] = p[2] * A[r][0] - p[0] * A[r][2];
        Hrr[r][2] = p[0] * A[r][1] - p[1] * A[r][0];
    }
    out[0] = Hrr[0][0]; out[1] = Hrr[0][1]; out[2] = Hrr[0][2]; out[3] = A[0][0]; out[4] = A[0][1]; out[5] = A[0][2];
    out[6] = Hrr[1][1]; out[7] = Hrr[1][2]; out[8] = A[1][0]; out[9] = A[1][1]; out[10] = A[1][2];
    out[11] = Hrr[2][2]; out[12] = A[2][0]; out[13] = A[2][1]; out[14] = A[2][2];
    out[15] = W[0]; out[16] = W[1]; out[17] = W[2]; out[18] = W[3]; out[19] = W[4]; out[20] = W[5];
    out[21] = p[1] * a.b[2] - p[2] * a.b[1];
    out[22] = p[2] * a.b[0] - p[0] * a.b[2];
    out[23] = p[0] * a.b[1] - p[1] * a.b[0];
    out[24] = a.b[0]; out[25] = a.b[1]; out[26] = a.b[2];
    out[S_SCORE] = a.s;
    out[S_WM] = a.sm;
    out[S_PAIRS] = (double)a.pairs;
    out[S_ROWS] = a.pairs > 0 ? 1.0 : 0.0;
    out[S_SINGULAR] = (double)a.singular;
}

// the scalar arguments of an evaluation: "" or why not
inline const char* check_scalars(const double* T, double cov_scale, double cov_floor) {
    if (!T) return "T is NULL";
    for (int i = 0; i < 16; ++i)
        if (!finite(T[i])) return "T is not finite";
    if (!(cov_scale > 0.0) || !finite(cov_scale)) return "cov_scale must be positive and finite";
    if (!(cov_floor >= 0.0) || !finite(cov_floor)) return "cov_floor must be non-negative and finite";
    return "";
}

}  // namespace d2d
}  // namespace gsr
