// model.hip -- level export glue on the device: scaling / rotation of every component of a mixture level
// from its covariance, behind gsr_decompose_cov (include/gsr_hip.h).
//
// Replaces GaussianModel.decompose_covariance_matrix + matrices_to_quaternions of the reference
// (src/models/gaussian_model.py:151-153,242-265, src/utils/general_utils.py:94-100), which run a batched
// torch.linalg.eigh, three gathers / scatters and a stack of element-wise kernels on "cuda:0" after every HEM level.
// One thread per component: float64 cyclic Jacobi on the symmetric 3x3 in registers (the covariances are float32; the
// decomposition is exact to float32 output precision), then
//
//   GSR_DECOMP_REFERENCE   the reference's arithmetic, bug for bug: eigenvalues ascending; eigenpair k claims the axis
//       its eigenvector is most aligned with (arg-max of |v_k|, first maximum on ties); the eigenVALUE k goes to that
//       slot of `scaling` and ROW k of the eigenvector matrix V (columns = eigenvectors; the reference scatters rows of
//       the tensor eigh returns, gaussian_model.py:262) goes to that row of the "rotation" matrix; two claims of one
//       slot overwrite in eigenvalue order (torch's CPU scatter_: the last one wins), an unclaimed slot stays zero;
//       quaternion (w, x, y, z) by the trace formula w = sqrt(1 + tr) / 2 without any branch (NaN when 1 + tr < 0, as
//       there).  The "scaling" is the eigenvalue itself -- not its square root, not a logarithm.
//   GSR_DECOMP_EXACT       what save_ply of a down-sampled model actually needs (the reference's own comment calls its
//       version unused): scaling = log of the standard deviations (0.5 log lambda_k, lambda clamped at 1e-30), rotation =
//       the proper rotation [v_0 v_1 v_2] (third column flipped if the determinant is negative) as a unit quaternion by
//       Shepperd's branch on the largest diagonal term, so that R diag(exp(scaling))^2 R^T reproduces the covariance.
//       A covariance with a NaN or infinite entry leaves as NaN in all three outputs (REFERENCE mode keeps the reference's
//       undefined behaviour there).
//
// Sign convention of the eigenvectors (torch.linalg.eigh leaves it to the LAPACK / rocSOLVER build): the component of
// largest magnitude of every eigenvector is positive (first maximum on ties).  Everything the reference path derives from
// V is invariant under column sign flips except the signs inside the scattered rows; tests compare up to those.
#include "gsr_common.h"
#include "gsr_covbuild.h"
#include "gsr_oneshot.h"

#include <float.h>
#include <math.h>
#include <string.h>

namespace gsr {

// cyclic Jacobi for a symmetric 3x3: A = V diag(lam) V^T, eigenvalues ascending, columns of V = eigenvectors
__device__ void sym_eig3_d(const double Ain[3][3], double V[3][3], double lam[3]) {
    double A[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { A[i][j] = Ain[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-34 * diag) || !(off == off)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {           // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {           // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {           // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
    // ascending order (three compare-exchanges on the columns)
    for (int pass = 0; pass < 3; ++pass) {
        const int a = pass == 1 ? 1 : 0, b = a + 1;             // (0,1) (1,2) (0,1)
        if (lam[b] < lam[a]) {
            const double t = lam[a]; lam[a] = lam[b]; lam[b] = t;
            for (int k = 0; k < 3; ++k) { const double v = V[k][a]; V[k][a] = V[k][b]; V[k][b] = v; }
        }
    }
    // sign convention: the component of largest magnitude of every eigenvector is positive
    for (int c = 0; c < 3; ++c) {
        int m = 0;
        if (fabs(V[1][c]) > fabs(V[m][c])) m = 1;
        if (fabs(V[2][c]) > fabs(V[m][c])) m = 2;
        if (V[m][c] < 0.0) for (int k = 0; k < 3; ++k) V[k][c] = -V[k][c];
    }
}

__global__ __launch_bounds__(256) void k_decompose_cov(int64_t n, const float* __restrict__ cov6, int mode, float* __restrict__ scaling,
                                                       float* __restrict__ quat, float* __restrict__ mat) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double c00 = cov6[6 * i], c01 = cov6[6 * i + 1], c02 = cov6[6 * i + 2], c11 = cov6[6 * i + 3], c12 = cov6[6 * i + 4], c22 = cov6[6 * i + 5];
        const double A[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
        double V[3][3], lam[3];
        sym_eig3_d(A, V, lam);
        float M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        float sc[3] = {0, 0, 0};
        float q[4];
        if (mode == GSR_DECOMP_REFERENCE) {
            for (int k = 0; k < 3; ++k) {                       // ascending eigenvalue: the later claim of a slot wins
                int slot = 0;                                   // arg-max of |v_k| = row k of |V^T| (gaussian_model.py:251-254)
                if (fabs(V[1][k]) > fabs(V[slot][k])) slot = 1;
                if (fabs(V[2][k]) > fabs(V[slot][k])) slot = 2;
                sc[slot] = (float)lam[k];
                for (int c = 0; c < 3; ++c) M[slot][c] = (float)V[k][c];      // ROW k of the eigenvector matrix, as the reference scatters it
            }
            const float w = sqrtf(1.0f + (M[0][0] + M[1][1] + M[2][2])) / 2.0f;      // general_utils.py:94-100
            q[0] = w;
            q[1] = (M[2][1] - M[1][2]) / (4.0f * w);
            q[2] = (M[0][2] - M[2][0]) / (4.0f * w);
            q[3] = (M[1][0] - M[0][1]) / (4.0f * w);
        } else {
            double R[3][3];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r][c] = V[r][c];
            const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                               R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
            if (det < 0.0) for (int r = 0; r < 3; ++r) R[r][2] = -R[r][2];
            for (int k = 0; k < 3; ++k) sc[k] = (float)(0.5 * log(lam[k] > 1e-30 ? lam[k] : 1e-30));
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = (float)R[r][c];
            // Shepperd: pick the largest of w^2, x^2, y^2, z^2
            const double tr = R[0][0] + R[1][1] + R[2][2];
            double w, x, y, z;
            if (tr > 0.0) {
                const double s = sqrt(tr + 1.0) * 2.0;
                w = 0.25 * s; x = (R[2][1] - R[1][2]) / s; y = (R[0][2] - R[2][0]) / s; z = (R[1][0] - R[0][1]) / s;
            } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
                const double s = sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]) * 2.0;
                w = (R[2][1] - R[1][2]) / s; x = 0.25 * s; y = (R[0][1] + R[1][0]) / s; z = (R[0][2] + R[2][0]) / s;
            } else if (R[1][1] > R[2][2]) {
                const double s = sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]) * 2.0;
                w = (R[0][2] - R[2][0]) / s; x = (R[0][1] + R[1][0]) / s; y = 0.25 * s; z = (R[1][2] + R[2][1]) / s;
            } else {
                const double s = sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]) * 2.0;
                w = (R[1][0] - R[0][1]) / s; x = (R[0][2] + R[2][0]) / s; y = (R[1][2] + R[2][1]) / s; z = 0.25 * s;
            }
            const double nq = sqrt(w * w + x * x + y * y + z * z);
            if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
            q[0] = (float)(w / nq); q[1] = (float)(x / nq); q[2] = (float)(y / nq); q[3] = (float)(z / nq);
            // a covariance with an entry that is not finite has no decomposition: the whole row leaves as NaN, not as the
            // plausible (V = I, lambda = diagonal) the broken-off Jacobi loop would hand on (x - x is NaN for NaN and +-Inf)
            if (!((c00 - c00) + (c01 - c01) + (c02 - c02) + (c11 - c11) + (c12 - c12) + (c22 - c22) == 0.0)) {
                const float nan = __builtin_nanf("");
                for (int k = 0; k < 3; ++k) sc[k] = nan;
                for (int k = 0; k < 4; ++k) q[k] = nan;
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = nan;
            }
        }
        scaling[3 * i] = sc[0]; scaling[3 * i + 1] = sc[1]; scaling[3 * i + 2] = sc[2];
        quat[4 * i] = q[0]; quat[4 * i + 1] = q[1]; quat[4 * i + 2] = q[2]; quat[4 * i + 3] = q[3];
        if (mat)
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) mat[9 * i + 3 * r + c] = M[r][c];
    }
}

// ---- RANSAC plane fitting: the data-parallel inner part of _fit_single_plane of the reference
// (src/utils/plane_fitting_util.py:38-69).  The reference evaluates its `iterations` candidate planes one after the
// other, each with five full-size torch kernels on the CPU; here ALL candidates of a plane search are scored in one
// pass over the points: a thread per point, the candidates broadcast from LDS, inliers counted per candidate by
// ballot + popcount (one LDS atomic per wave and candidate).
//   distance  = (x n'_0 + y n'_1 + z n'_2 + d) / |n'|      n' = the plane normal re-normalised in float32 (:91-96)
//   inlier   <=> |distance| < distance_threshold  and  |<point normal, plane normal>| > normal_threshold   (:54-61)
// float32 throughout.  The reference's dot products come out of torch.mm / torch.matmul on the CPU, i.e. MKL's sgemv, whose
// K = 3 rows round as  fl(z n2) + fma(y, n1, fl(x n0))  -- measured in the build container: that expression reproduces
// torch.mm bit for bit on 10^6 random rows, EXCEPT the few rows in the tail of each OpenMP thread's share (266 of 2.3 M rows
// with 8 threads; which rows depends on the thread count of the machine), which take another path.  So the host result
// cannot be reproduced exactly in general; the kernel uses the dominant rounding (tests/test_planes_gpu.py).
struct PlaneCand { float n0, n1, n2, d, m0, m1, m2, nn; };      // n' (re-normalised), d, plane normal as sampled, |n'|

__device__ __forceinline__ bool plane_inlier(const PlaneCand& c, float x, float y, float z, float nx, float ny, float nz, float dist_thr, float nrm_thr) {
    const float dot = z * c.n2 + __builtin_fmaf(y, c.n1, x * c.n0);
    const float dist = (dot + c.d) / c.nn;
    const float al = nz * c.m2 + __builtin_fmaf(ny, c.m1, nx * c.m0);
    return fabsf(dist) < dist_thr && fabsf(al) > nrm_thr;
}

#define PLANE_CHUNK 256
__global__ __launch_bounds__(256) void k_plane_score(int64_t n, const float* __restrict__ xyz, const float* __restrict__ nrm, int P,
                                                     const PlaneCand* __restrict__ cand, float dist_thr, float nrm_thr, unsigned* __restrict__ counts) {
    __shared__ PlaneCand s_c[PLANE_CHUNK];
    __shared__ unsigned s_n[PLANE_CHUNK];
    const int lane = threadIdx.x & 63;
    for (int p0 = 0; p0 < P; p0 += PLANE_CHUNK) {
        const int pn = P - p0 < PLANE_CHUNK ? P - p0 : PLANE_CHUNK;
        __syncthreads();
        if ((int)threadIdx.x < pn) { s_c[threadIdx.x] = cand[p0 + threadIdx.x]; s_n[threadIdx.x] = 0u; }
        __syncthreads();
        for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = i0 + threadIdx.x;
            const bool live = i < n;
            const int64_t ii = live ? i : 0;
            const float x = xyz[3 * ii], y = xyz[3 * ii + 1], z = xyz[3 * ii + 2];
            const float nx = nrm[3 * ii], ny = nrm[3 * ii + 1], nz = nrm[3 * ii + 2];
            for (int p = 0; p < pn; ++p) {
                const bool in = live && plane_inlier(s_c[p], x, y, z, nx, ny, nz, dist_thr, nrm_thr);
                const unsigned long long m = __ballot(in);
                if (m != 0ull && lane == 0) atomicAdd(&s_n[p], (unsigned)__popcll(m));
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < pn && s_n[threadIdx.x]) atomicAdd(&counts[p0 + threadIdx.x], s_n[threadIdx.x]);
    }
}
__global__ __launch_bounds__(256) void k_plane_mask(int64_t n, const float* __restrict__ xyz, const float* __restrict__ nrm, PlaneCand c,
                                                    float dist_thr, float nrm_thr, uint8_t* __restrict__ mask) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = plane_inlier(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], dist_thr, nrm_thr) ? 1 : 0;
}

// ---- rigid motion of a splat model in one pass (gsr_model_transform) ---------------------------------------------------------
// The last stage of the pipeline (GaussianModel.transform_gaussian_model / get_merged_gaussian_point_clouds): positions,
// covariances, orientation quaternions and -- what the torch chain never did -- the view-dependent colour, i.e. the SH-rest
// coefficients, which transform band by band with the matrices D_1 (3x3), D_2 (5x5), D_3 (7x7) of gsr_sh_rotation.
//
// SH basis = the one 3DGS evaluates (its published forward pass), coefficient k of _features_rest[n, k, c]:
//   band 1: -C1 y, C1 z, -C1 x
//   band 2: C2[0] xy, C2[1] yz, C2[2] (2zz - xx - yy), C2[3] xz, C2[4] (xx - yy)
//   band 3: C3[0] y(3xx - yy), C3[1] xyz, C3[2] y(4zz - xx - yy), C3[3] z(2zz - 3xx - 3yy), C3[4] x(4zz - xx - yy), C3[5] z(xx - yy),
//           C3[6] x(xx - 3yy)
// D_l is defined by  basis_l(R d) . (D_l c) = basis_l(d) . c  for every direction d and coefficient vector c: the rotated splat
// seen from the rotated direction shows the original colour.  The basis is orthonormal on the sphere, so D_l is orthogonal and
// basis_l(R d) = D_l basis_l(d); gsr_sh_rotation fits exactly that by least squares over a fixed set of directions (host, float64).
static const double SH_C1 = 0.4886025119029199;
static const double SH_C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
static const double SH_C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                                1.445305721320277, -0.5900435899266435};

// the 15 rest basis functions at the unit direction (x, y, z), band after band
static void sh_basis_rest(double x, double y, double z, double* b) {
    const double xx = x * x, yy = y * y, zz = z * z;
    b[0] = -SH_C1 * y; b[1] = SH_C1 * z; b[2] = -SH_C1 * x;
    b[3] = SH_C2[0] * x * y; b[4] = SH_C2[1] * y * z; b[5] = SH_C2[2] * (2.0 * zz - xx - yy); b[6] = SH_C2[3] * x * z; b[7] = SH_C2[4] * (xx - yy);
    b[8] = SH_C3[0] * y * (3.0 * xx - yy); b[9] = SH_C3[1] * x * y * z; b[10] = SH_C3[2] * y * (4.0 * zz - xx - yy);
    b[11] = SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy); b[12] = SH_C3[4] * x * (4.0 * zz - xx - yy); b[13] = SH_C3[5] * z * (xx - yy);
    b[14] = SH_C3[6] * x * (xx - 3.0 * yy);
}

// X <- A^-1 X for a well-conditioned m x m system with m right-hand sides (Gaussian elimination, partial pivoting); false if singular
static bool solve_in_place(int m, double A[7][7], double X[7][7]) {
    for (int c = 0; c < m; ++c) {
        int piv = c;
        for (int r = c + 1; r < m; ++r) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (!(fabs(A[piv][c]) > 1e-12)) return false;
        if (piv != c) for (int k = 0; k < m; ++k) { double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; t = X[c][k]; X[c][k] = X[piv][k]; X[piv][k] = t; }
        for (int r = 0; r < m; ++r) {
            if (r == c) continue;
            const double f = A[r][c] / A[c][c];
            if (f == 0.0) continue;
            for (int k = 0; k < m; ++k) { A[r][k] -= f * A[c][k]; X[r][k] -= f * X[c][k]; }
        }
    }
    for (int r = 0; r < m; ++r) for (int k = 0; k < m; ++k) X[r][k] /= A[r][r];
    return true;
}

// the rotation matrices of the three rest bands in float32, as the kernel takes them BY VALUE (kernel arguments are read with
// scalar loads: the 83 values are wave-uniform and never cost a per-lane global read)
struct ShRot { float d1[9], d2[25], d3[49]; };
// rotation, translation, unit quaternion (w, x, y, z) of the rotation; c, c2 = c^2, lnc = ln c: the factor of a similarity, read by
// the SIM instantiations only (gsr_model_similarity) -- the rigid ones never touch them
struct Rigid { float R[9], t[3], q[4], c, c2, lnc; };

// one channel's band vector of length M = 2l + 1 at s[0], s[3], s[6], ... (coefficient-major, channel-minor) <- D s
template <int M> __device__ __forceinline__ void sh_band(const float* __restrict__ D, float* s) {
    float v[M], o[M];
#pragma unroll
    for (int j = 0; j < M; ++j) v[j] = s[3 * j];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        float a = D[M * i] * v[0];
#pragma unroll
        for (int j = 1; j < M; ++j) a = __builtin_fmaf(D[M * i + j], v[j], a);
        o[i] = a;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) s[3 * i] = o[i];
}

// xyz' = R xyz + t;  cov' = R cov R^T on the six-entry form;  q' = normalise(q_R (x) q), a thread per splat.
// SIM: xyz' = c (R xyz) + t, cov' = c^2 (R cov R^T) -- one more float32 multiply each, behind the rigid expression -- and the
// log-scales scl' = scl + ln c (scl may be NULL).
template <bool SIM>
__device__ __forceinline__ void transform_geometry(int64_t n, const Rigid& G, const float* __restrict__ xyz, const float* __restrict__ cov6,
                                                   const float* __restrict__ rot, float* __restrict__ xyz_o, float* __restrict__ cov6_o,
                                                   float* __restrict__ rot_o, const float* __restrict__ scl = nullptr, float* __restrict__ scl_o = nullptr) {
    const float* R = G.R;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float m = __builtin_fmaf(R[3 * r + 2], z, __builtin_fmaf(R[3 * r + 1], y, R[3 * r] * x));
            xyz_o[3 * i + r] = (SIM ? G.c * m : m) + G.t[r];
        }
        const float c00 = cov6[6 * i], c01 = cov6[6 * i + 1], c02 = cov6[6 * i + 2], c11 = cov6[6 * i + 3], c12 = cov6[6 * i + 4], c22 = cov6[6 * i + 5];
        float M[3][3];                                  // M = R cov
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            M[r][0] = __builtin_fmaf(R[3 * r + 2], c02, __builtin_fmaf(R[3 * r + 1], c01, R[3 * r] * c00));
            M[r][1] = __builtin_fmaf(R[3 * r + 2], c12, __builtin_fmaf(R[3 * r + 1], c11, R[3 * r] * c01));
            M[r][2] = __builtin_fmaf(R[3 * r + 2], c22, __builtin_fmaf(R[3 * r + 1], c12, R[3 * r] * c02));
        }
        int o = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) {               // (M R^T)[r][c], upper triangle in the order xx xy xz yy yz zz
                const float v = __builtin_fmaf(M[r][2], R[3 * c + 2], __builtin_fmaf(M[r][1], R[3 * c + 1], M[r][0] * R[3 * c]));
                cov6_o[6 * i + o++] = SIM ? G.c2 * v : v;
            }
        if (SIM && scl) {
#pragma unroll
            for (int r = 0; r < 3; ++r) scl_o[3 * i + r] = scl[3 * i + r] + G.lnc;
        }
        if (rot) {
            const float w0 = rot[4 * i], x0 = rot[4 * i + 1], y0 = rot[4 * i + 2], z0 = rot[4 * i + 3];
            const float w1 = G.q[0], x1 = G.q[1], y1 = G.q[2], z1 = G.q[3];
            const float qw = w1 * w0 - x1 * x0 - y1 * y0 - z1 * z0;          // Hamilton product, motion on the left (gaussian_model.py)
            const float qx = w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0;
            const float qy = w1 * y0 - x1 * z0 + y1 * w0 + z1 * x0;
            const float qz = w1 * z0 + x1 * y0 - y1 * x0 + z1 * w0;
            const float nq = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
            rot_o[4 * i] = qw / nq; rot_o[4 * i + 1] = qx / nq; rot_o[4 * i + 2] = qy / nq; rot_o[4 * i + 3] = qz / nq;
        }
    }
}

// Geometry + SH in one launch.  The SH block is the traffic (4 F bytes in and out per splat, F = 3K = 45 floats at degree 3 against 52
// for everything else): a block's 256 rows are ONE contiguous run of 256 F floats, moved between HBM and LDS with full-width
// coalesced accesses (dwordx4 when VEC and the arrays are 16-byte aligned, every tile start then is too); in between each lane owns
// one row of the LDS image.  Row stride FP = F or F + 1, always odd: the 32 lanes of a ds_read_b32 / ds_write_b32 group then fall on
// 32 different banks.  The row is transformed in place in LDS (a lane reads and writes only its own row), so the image is loaded,
// rotated and stored with three barriers per tile and no second buffer: 256 x 45 x 4 = 45 KiB at degree 3, three blocks per CU.
template <int K, bool VEC, bool SIM>
__global__ __launch_bounds__(256) void k_model_transform(int64_t n, Rigid G, ShRot D, const float* __restrict__ xyz, const float* __restrict__ cov6,
                                                         const float* __restrict__ rot, const float* __restrict__ sh, float* __restrict__ xyz_o,
                                                         float* __restrict__ cov6_o, float* __restrict__ rot_o, float* __restrict__ sh_o,
                                                         const float* __restrict__ scl, float* __restrict__ scl_o) {
    constexpr int F = 3 * K, FP = F | 1, ROWS = 256;
    __shared__ float s_sh[ROWS * FP];
    const int tid = threadIdx.x;
    const int64_t tiles = (n + ROWS - 1) / ROWS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {          // uniform over the block: the barriers are legal
        const int64_t row0 = tile * ROWS;
        const int rows = n - row0 < ROWS ? (int)(n - row0) : ROWS;
        const int cnt = rows * F;                                               // floats of this tile, contiguous from row0 * F
        const float* __restrict__ src = sh + row0 * F;
        float* __restrict__ dst = sh_o + row0 * F;
        if (VEC) {
            const int nv = cnt >> 2;
            for (int v = tid; v < nv; v += 256) {
                const float4 q = reinterpret_cast<const float4*>(src)[v];
                const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int f = 4 * v + j, r = f / F; s_sh[r * FP + (f - r * F)] = e[j]; }
            }
            for (int f = 4 * nv + tid; f < cnt; f += 256) { const int r = f / F; s_sh[r * FP + (f - r * F)] = src[f]; }
        } else {
            for (int f = tid; f < cnt; f += 256) { const int r = f / F; s_sh[r * FP + (f - r * F)] = src[f]; }
        }
        __syncthreads();
        if (tid < rows) {
            float* s = s_sh + tid * FP;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sh_band<3>(D.d1, s + c);
                if (K >= 8) sh_band<5>(D.d2, s + 9 + c);
                if (K >= 15) sh_band<7>(D.d3, s + 24 + c);
            }
        }
        __syncthreads();
        if (VEC) {
            const int nv = cnt >> 2;
            for (int v = tid; v < nv; v += 256) {
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int f = 4 * v + j, r = f / F; e[j] = s_sh[r * FP + (f - r * F)]; }
                reinterpret_cast<float4*>(dst)[v] = make_float4(e[0], e[1], e[2], e[3]);
            }
            for (int f = 4 * nv + tid; f < cnt; f += 256) { const int r = f / F; dst[f] = s_sh[r * FP + (f - r * F)]; }
        } else {
            for (int f = tid; f < cnt; f += 256) { const int r = f / F; dst[f] = s_sh[r * FP + (f - r * F)]; }
        }
        __syncthreads();                                                        // the next tile overwrites the image
    }
    transform_geometry<SIM>(n, G, xyz, cov6, rot, xyz_o, cov6_o, rot_o, scl, scl_o);
}

// the same without SH rotation: `words` 32-bit words of sh copied bit for bit (as integers: no float ever touches them)
template <bool VEC, bool SIM>
__global__ __launch_bounds__(256) void k_model_transform_copy(int64_t n, Rigid G, int64_t words, const float* __restrict__ xyz, const float* __restrict__ cov6,
                                                              const float* __restrict__ rot, const uint32_t* __restrict__ sh, float* __restrict__ xyz_o,
                                                              float* __restrict__ cov6_o, float* __restrict__ rot_o, uint32_t* __restrict__ sh_o,
                                                              const float* __restrict__ scl, float* __restrict__ scl_o) {
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (VEC) {
        const int64_t nv = words >> 2;
        for (int64_t v = t0; v < nv; v += step) reinterpret_cast<uint4*>(sh_o)[v] = reinterpret_cast<const uint4*>(sh)[v];
        for (int64_t f = 4 * nv + t0; f < words; f += step) sh_o[f] = sh[f];
    } else {
        for (int64_t f = t0; f < words; f += step) sh_o[f] = sh[f];
    }
    transform_geometry<SIM>(n, G, xyz, cov6, rot, xyz_o, cov6_o, rot_o, scl, scl_o);
}

// ---- device SoA -> 3DGS .ply rows (gsr_ply_pack), the inverse of k_ply_unpack ------------------------------------------------
// A thread per output float, consecutive threads on consecutive addresses of the row image: x y z, three zero normals, f_dc_0..2,
// f_rest channel-major (file f_rest[c * K + k] = sh[i][k][c]), opacity, scale_0..2, rot_0..3 -- 17 + 3K little-endian float32 per row,
// what save_gaussian_ply writes.  The reads of one row come from six arrays but stay inside that row's own few cache lines.
__global__ __launch_bounds__(256) void k_ply_pack(int64_t n, int K, const float* __restrict__ xyz, const float* __restrict__ dc, const float* __restrict__ sh,
                                                  const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ rot,
                                                  float* __restrict__ rows) {
    const int F = 3 * K, W = 17 + F;
    const int64_t total = n * W;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / W;
        const int j = (int)(t - i * W);
        float v;
        if (j < 3) v = xyz[3 * i + j];
        else if (j < 6) v = 0.0f;
        else if (j < 9) v = dc[3 * i + (j - 6)];
        else if (j < 9 + F) { const int f = j - 9, c = f / K, k = f - c * K; v = sh[i * F + 3 * k + c]; }
        else if (j == 9 + F) v = opacity[i];
        else if (j < 13 + F) v = scale[3 * i + (j - 10 - F)];
        else v = rot[4 * i + (j - 13 - F)];
        rows[t] = v;
    }
}

}  // namespace gsr

using namespace gsr;

// ---- gsr_sh_rotation: host only ----------------------------------------------------------------------------------------------
static bool rotation_ok(const double* R) {
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = i == j ? -1.0 : 0.0;
            for (int k = 0; k < 3; ++k) d += R[3 * k + i] * R[3 * k + j];
            if (!(fabs(d) <= worst)) worst = fabs(d);                   // a NaN sticks
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return worst <= 1e-3 && det > 0.0;
}

extern "C" int32_t gsr_sh_rotation(const double* rotation, int32_t degree, double* bands) {
    if (!rotation || !bands) return fail(GSR_E_INVALID, "gsr_sh_rotation: NULL argument");
    if (degree < 0 || degree > 3) return fail(GSR_E_INVALID, "gsr_sh_rotation: SH degree %d outside 0..3", degree);
    if (!rotation_ok(rotation)) return fail(GSR_E_INVALID, "gsr_sh_rotation: the 3x3 is not a rotation (max|R^T R - I| > 1e-3 or det < 0)");
    // sample directions: a Fibonacci spiral, well spread, so the normal matrix of every band is close to a multiple of the identity
    const int S = 96;
    double Y[S][15], Z[S][15];
    for (int s = 0; s < S; ++s) {
        const double z = 1.0 - (2.0 * s + 1.0) / S, r = sqrt(1.0 - z * z), phi = 2.399963229728653 * s;
        const double d[3] = {r * cos(phi), r * sin(phi), z};
        double e[3];
        for (int i = 0; i < 3; ++i) e[i] = rotation[3 * i] * d[0] + rotation[3 * i + 1] * d[1] + rotation[3 * i + 2] * d[2];
        const double ne = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        sh_basis_rest(d[0], d[1], d[2], Y[s]);
        sh_basis_rest(e[0] / ne, e[1] / ne, e[2] / ne, Z[s]);
    }
    const int off[3] = {0, 3, 8}, out[3] = {0, 9, 34};
    for (int l = 1; l <= 3; ++l) {
        const int m = 2 * l + 1, o = off[l - 1];
        double* D = bands + out[l - 1];
        if (l > degree) {                                               // bands the model does not carry: the identity
            for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) D[m * i + j] = i == j ? 1.0 : 0.0;
            continue;
        }
        // Z = Y D^T in the least-squares sense:  (Y^T Y) D^T = Y^T Z
        double A[7][7], X[7][7];
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                double a = 0.0, x = 0.0;
                for (int s = 0; s < S; ++s) { a += Y[s][o + i] * Y[s][o + j]; x += Y[s][o + i] * Z[s][o + j]; }
                A[i][j] = a; X[i][j] = x;
            }
        if (!solve_in_place(m, A, X)) return fail(GSR_E_INVALID, "gsr_sh_rotation: singular fit in band %d", l);
        for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) D[m * i + j] = X[j][i];
    }
    return GSR_OK;
}

// ---- gsr_model_transform -----------------------------------------------------------------------------------------------------
template <int K, bool SIM> static void launch_model_transform(bool vec, int grid, hipStream_t st, int64_t n, const Rigid& G, const ShRot& D, const float* xyz,
                                                              const float* cov6, const float* rot, const float* sh, float* xyz_o, float* cov6_o, float* rot_o, float* sh_o,
                                                              const float* scl, float* scl_o) {
    if (vec) hipLaunchKernelGGL((k_model_transform<K, true, SIM>), dim3(grid), dim3(256), 0, st, n, G, D, xyz, cov6, rot, sh, xyz_o, cov6_o, rot_o, sh_o, scl, scl_o);
    else hipLaunchKernelGGL((k_model_transform<K, false, SIM>), dim3(grid), dim3(256), 0, st, n, G, D, xyz, cov6, rot, sh, xyz_o, cov6_o, rot_o, sh_o, scl, scl_o);
}

// The similarity gate: det A > 0, c = cbrt(det A) in [1e-6, 1e6], max|A^T A / c^2 - I| <= 1e-3.  R9 = A / c (float64).
static bool similarity_ok(const double* A, double* c_out, double* R9) {
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (!(det > 0.0)) return false;
    const double c = cbrt(det);
    if (!(c >= 1e-6 && c <= 1e6)) return false;
    for (int i = 0; i < 9; ++i) R9[i] = A[i] / c;
    *c_out = c;
    return rotation_ok(R9);
}

// gsr_model_transform (SIM = false: c = 1, no scaling arrays) and gsr_model_similarity (SIM = true) behind their gates
template <bool SIM>
static int32_t model_move(const char* who, const double* transform, const double* R9, double c, int64_t n, int32_t K, int32_t rotate_sh, const float* xyz,
                          const float* cov6, const float* rot, const float* sh, const float* scaling, float* xyz_out, float* cov6_out, float* rot_out,
                          float* sh_out, float* scaling_out, int32_t on_device, int32_t device, void* stream) {
    const size_t un = (size_t)n, F = 3 * (size_t)K;
    const size_t bytes[5] = {un * 12, un * 24, un * 16, un * F * 4, un * 12};
    const ByteRange ins[5] = {{xyz, bytes[0]}, {cov6, bytes[1]}, {rot, bytes[2]}, {K ? sh : nullptr, bytes[3]}, {scaling, bytes[4]}};
    const ByteRange outs[5] = {{xyz_out, bytes[0]}, {cov6_out, bytes[1]}, {rot ? rot_out : nullptr, bytes[2]}, {K ? sh_out : nullptr, bytes[3]},
                               {scaling ? scaling_out : nullptr, bytes[4]}};
    if (!outputs_disjoint(outs, 5, ins, 5))
        return fail(GSR_E_INVALID, "%s: an output array overlaps another array of the call (the transform is not in place)", who);
    GSR_TRY(open_device(device, who));
    if (n == 0) return GSR_OK;
    // the motion narrowed to float32 once: rotation, translation, the rotation's unit quaternion (Shepperd's branch, w >= 0)
    Rigid G;
    for (int i = 0; i < 9; ++i) G.R[i] = (float)R9[i];
    for (int i = 0; i < 3; ++i) G.t[i] = (float)transform[4 * i + 3];
    G.c = (float)c; G.c2 = (float)(c * c); G.lnc = (float)log(c);
    {
        const double* R = R9;
        const double tr = R[0] + R[4] + R[8];
        double w, x, y, z;
        if (tr > 0.0) { const double s = sqrt(tr + 1.0) * 2.0; w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s; }
        else if (R[0] > R[4] && R[0] > R[8]) { const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0; w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s; }
        else if (R[4] > R[8]) { const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0; w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s; }
        else { const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0; w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s; }
        const double nq = sqrt(w * w + x * x + y * y + z * z) * (w < 0.0 ? -1.0 : 1.0);
        G.q[0] = (float)(w / nq); G.q[1] = (float)(x / nq); G.q[2] = (float)(y / nq); G.q[3] = (float)(z / nq);
    }
    ShRot D;
    memset(&D, 0, sizeof(D));
    const bool rotate = rotate_sh != 0 && K > 0;
    if (rotate) {
        double B[83];
        GSR_TRY(gsr_sh_rotation(R9, K == 3 ? 1 : K == 8 ? 2 : 3, B));
        for (int i = 0; i < 9; ++i) D.d1[i] = (float)B[i];
        for (int i = 0; i < 25; ++i) D.d2[i] = (float)B[9 + i];
        for (int i = 0; i < 49; ++i) D.d3[i] = (float)B[34 + i];
    }
    OneShot os((hipStream_t)stream, on_device != 0, who);
    const float *px = nullptr, *pc = nullptr, *pq = nullptr, *ps = nullptr, *pl = nullptr;
    float *ox = nullptr, *oc = nullptr, *oq = nullptr, *osh = nullptr, *ol = nullptr;
    GSR_TRY(os.in(xyz, bytes[0], &px));
    GSR_TRY(os.in(cov6, bytes[1], &pc));
    GSR_TRY(os.in(rot, bytes[2], &pq));
    GSR_TRY(os.in(K ? sh : nullptr, bytes[3], &ps));
    if (SIM) GSR_TRY(os.in(scaling, bytes[4], &pl));
    GSR_TRY(os.out(xyz_out, bytes[0], &ox));
    GSR_TRY(os.out(cov6_out, bytes[1], &oc));
    GSR_TRY(os.out(rot ? rot_out : nullptr, bytes[2], &oq));
    GSR_TRY(os.out(K ? sh_out : nullptr, bytes[3], &osh));
    if (SIM) GSR_TRY(os.out(scaling ? scaling_out : nullptr, bytes[4], &ol));
    const bool vec = (((uintptr_t)ps | (uintptr_t)osh) & 15u) == 0u;
    if (rotate) {
        const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);        // a block per 256-row tile, at most 16 per CU
        if (K == 3) launch_model_transform<3, SIM>(vec, grid, os.st, n, G, D, px, pc, pq, ps, ox, oc, oq, osh, pl, ol);
        else if (K == 8) launch_model_transform<8, SIM>(vec, grid, os.st, n, G, D, px, pc, pq, ps, ox, oc, oq, osh, pl, ol);
        else launch_model_transform<15, SIM>(vec, grid, os.st, n, G, D, px, pc, pq, ps, ox, oc, oq, osh, pl, ol);
    } else {
        const int64_t words = n * (int64_t)F;
        const int grid = stride_grid(words > 4 * n ? words / 4 : n);
        if (vec) hipLaunchKernelGGL((k_model_transform_copy<true, SIM>), dim3(grid), dim3(256), 0, os.st, n, G, words, px, pc, pq, (const uint32_t*)ps, ox, oc, oq, (uint32_t*)osh, pl, ol);
        else hipLaunchKernelGGL((k_model_transform_copy<false, SIM>), dim3(grid), dim3(256), 0, os.st, n, G, words, px, pc, pq, (const uint32_t*)ps, ox, oc, oq, (uint32_t*)osh, pl, ol);
    }
    return os.finish();
}

extern "C" int32_t gsr_model_transform(const double* transform, int64_t n, int32_t K, int32_t rotate_sh, const float* xyz, const float* cov6,
                                       const float* rot, const float* sh, float* xyz_out, float* cov6_out, float* rot_out, float* sh_out,
                                       int32_t on_device, int32_t device, void* stream) {
    if (!transform || n < 0 || (K != 0 && K != 3 && K != 8 && K != 15)) return fail(GSR_E_INVALID, "gsr_model_transform: bad argument (K must be 0, 3, 8 or 15)");
    if (n > 0 && (!xyz || !cov6 || !xyz_out || !cov6_out || (rot && !rot_out) || (K > 0 && (!sh || !sh_out))))
        return fail(GSR_E_INVALID, "gsr_model_transform: NULL array");
    const double R9[9] = {transform[0], transform[1], transform[2], transform[4], transform[5], transform[6], transform[8], transform[9], transform[10]};
    if (!rotation_ok(R9)) return fail(GSR_E_INVALID, "gsr_model_transform: the upper 3x3 of the transform is not a rotation");
    return model_move<false>("gsr_model_transform", transform, R9, 1.0, n, K, rotate_sh, xyz, cov6, rot, sh, nullptr, xyz_out, cov6_out, rot_out, sh_out, nullptr,
                             on_device, device, stream);
}

extern "C" int32_t gsr_model_similarity(const double* transform, int64_t n, int32_t K, int32_t rotate_sh, const float* xyz, const float* cov6,
                                        const float* rot, const float* sh, const float* scaling, float* xyz_out, float* cov6_out, float* rot_out,
                                        float* sh_out, float* scaling_out, int32_t on_device, int32_t device, void* stream) {
    if (!transform || n < 0 || (K != 0 && K != 3 && K != 8 && K != 15)) return fail(GSR_E_INVALID, "gsr_model_similarity: bad argument (K must be 0, 3, 8 or 15)");
    if (n > 0 && (!xyz || !cov6 || !xyz_out || !cov6_out || (rot && !rot_out) || (scaling && !scaling_out) || (K > 0 && (!sh || !sh_out))))
        return fail(GSR_E_INVALID, "gsr_model_similarity: NULL array");
    const double A9[9] = {transform[0], transform[1], transform[2], transform[4], transform[5], transform[6], transform[8], transform[9], transform[10]};
    double c = 1.0, R9[9];
    if (!similarity_ok(A9, &c, R9))
        return fail(GSR_E_INVALID, "gsr_model_similarity: the upper 3x3 of the transform is not c R (det > 0, 1e-6 <= c <= 1e6, max|A^T A / c^2 - I| <= 1e-3)");
    return model_move<true>("gsr_model_similarity", transform, R9, c, n, K, rotate_sh, xyz, cov6, rot, sh, scaling, xyz_out, cov6_out, rot_out, sh_out, scaling_out,
                            on_device, device, stream);
}

extern "C" int32_t gsr_ply_pack(const float* xyz, const float* dc, const float* sh, const float* opacity, const float* scale, const float* rot,
                                int64_t n, int32_t K, void* rows_dev, int32_t device, void* stream) {
    if (n < 0 || K < 0 || K > 1024 || (n > 0 && (!xyz || !dc || !opacity || !scale || !rot || !rows_dev || (K > 0 && !sh))))
        return fail(GSR_E_INVALID, "gsr_ply_pack: bad argument");
    GSR_TRY(open_device(device, "gsr_ply_pack"));
    if (n == 0) return GSR_OK;
    hipLaunchKernelGGL(k_ply_pack, dim3(stride_grid(n * (17 + 3 * (int64_t)K))), dim3(256), 0, (hipStream_t)stream, n, (int)K, xyz, dc, sh, opacity, scale, rot,
                       (float*)rows_dev);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

extern "C" int32_t gsr_plane_score(const float* xyz, const float* normals, int64_t n, const float* candidates, int32_t n_candidates,
                                   float distance_threshold, float normal_threshold, uint32_t* counts, uint8_t* best_mask, int32_t* best,
                                   int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || n_candidates < 0 || (n > 0 && (!xyz || !normals)) || (n_candidates > 0 && (!candidates || !counts)) || !best)
        return fail(GSR_E_INVALID, "gsr_plane_score: bad argument");
    GSR_TRY(open_device(device, "gsr_plane_score"));
    *best = -1;
    if (n == 0 || n_candidates == 0) return GSR_OK;
    static_assert(sizeof(PlaneCand) == 32, "candidates are 8 floats");
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_plane_score");
    const float *px = nullptr, *pn = nullptr;
    PlaneCand* dc = nullptr;            // candidates and counts are host arrays in either placement
    unsigned* dcnt = nullptr;
    uint8_t* dm = nullptr;
    GSR_TRY(os.scratch((size_t)n_candidates * 32, &dc));
    GSR_TRY(os.scratch((size_t)n_candidates * 4, &dcnt));
    GSR_TRY(os.in(xyz, (size_t)n * 12, &px));
    GSR_TRY(os.in(normals, (size_t)n * 12, &pn));
    GSR_TRY(os.out(best_mask, (size_t)n, &dm));
    GSR_HIP(hipMemcpyAsync(dc, candidates, (size_t)n_candidates * 32, hipMemcpyHostToDevice, os.st));
    GSR_HIP(hipMemsetAsync(dcnt, 0, (size_t)n_candidates * 4, os.st));
    hipLaunchKernelGGL(k_plane_score, dim3(stride_grid(n)), dim3(256), 0, os.st, n, px, pn, (int)n_candidates, dc, distance_threshold, normal_threshold, dcnt);
    GSR_HIP(hipMemcpyAsync(counts, dcnt, (size_t)n_candidates * 4, hipMemcpyDeviceToHost, os.st));
    GSR_TRY(os.wait());
    // the reference keeps the FIRST candidate with the strictly largest count (plane_fitting_util.py:63-66)
    uint32_t mx = 0;
    for (int32_t p = 0; p < n_candidates; ++p)
        if (counts[p] > mx) { mx = counts[p]; *best = p; }
    if (*best < 0 || !best_mask) return GSR_OK;
    PlaneCand c;
    memcpy(&c, candidates + 8 * (size_t)*best, sizeof(c));
    hipLaunchKernelGGL(k_plane_mask, dim3(stride_grid(n)), dim3(256), 0, os.st, n, px, pn, c, distance_threshold, normal_threshold, dm);
    return os.finish();
}

// ---- 3DGS .ply rows -> device SoA ------------------------------------------------------------------------
// The reference loads a .ply straight onto cuda:0 (src/models/gaussian_model.py:98-139: plyfile -> numpy -> torch.tensor(device=
// "cuda"), the f_rest block transposed from the file's channel-major (P, 3, K) to coefficient-major (P, K, 3), the covariance
// built there from scale and rotation, :34-38,139).  Here the file's vertex rows (little-endian float32 properties, any order:
// `off` holds each wanted property's byte offset inside a row) arrive in HBM as they are on disk -- chunked through pinned
// memory by the host -- and ONE kernel scatters a chunk into the level-0 arrays the HEM boundary takes.
struct PlyLayout {
    int row_bytes;
    int K;                      // SH-rest coefficients per channel (15 at degree 3)
    int xyz[3], dc[3], opacity, scale[3], rot[4];
    int rest0;                  // byte offset of f_rest_0 ... f_rest_(3K-1), consecutive float32
};

__device__ __forceinline__ float ply_f32(const unsigned char* row, int off) {
    float v;
    if ((reinterpret_cast<uintptr_t>(row + off) & 3u) == 0u) v = *reinterpret_cast<const float*>(row + off);
    else memcpy(&v, row + off, 4);              // rows of files with uchar / double properties in front need not be 4-byte aligned
    return v;
}

__global__ __launch_bounds__(256) void k_ply_unpack(int64_t n, const unsigned char* __restrict__ rows, PlyLayout L, float* __restrict__ xyz,
                                                    float* __restrict__ color, float* __restrict__ sh, float* __restrict__ opacity,
                                                    float* __restrict__ scale, float* __restrict__ rot, float* __restrict__ cov6) {
    const int F = 3 * L.K;
    // geometry: a thread per splat
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned char* r = rows + i * L.row_bytes;
        xyz[3 * i] = ply_f32(r, L.xyz[0]); xyz[3 * i + 1] = ply_f32(r, L.xyz[1]); xyz[3 * i + 2] = ply_f32(r, L.xyz[2]);
        color[3 * i] = ply_f32(r, L.dc[0]); color[3 * i + 1] = ply_f32(r, L.dc[1]); color[3 * i + 2] = ply_f32(r, L.dc[2]);
        opacity[i] = ply_f32(r, L.opacity);
        const float s0 = ply_f32(r, L.scale[0]), s1 = ply_f32(r, L.scale[1]), s2 = ply_f32(r, L.scale[2]);
        const float qw = ply_f32(r, L.rot[0]), qx = ply_f32(r, L.rot[1]), qy = ply_f32(r, L.rot[2]), qz = ply_f32(r, L.rot[3]);
        scale[3 * i] = s0; scale[3 * i + 1] = s1; scale[3 * i + 2] = s2;
        rot[4 * i] = qw; rot[4 * i + 1] = qx; rot[4 * i + 2] = qy; rot[4 * i + 3] = qz;
        // build_rotation (general_utils.py:43-66) on the normalised quaternion, L = R diag(exp(scale)), covariance = L L^T (:69-80), float32
        float c[6];
        cov_build(s0, s1, s2, qw, qx, qy, qz, c);
        cov6[6 * i] = c[0]; cov6[6 * i + 1] = c[1]; cov6[6 * i + 2] = c[2]; cov6[6 * i + 3] = c[3]; cov6[6 * i + 4] = c[4]; cov6[6 * i + 5] = c[5];
    }
    // SH rest: a thread per output float, consecutive threads on consecutive output addresses; sh[i][k][c] = file f_rest[c * K + k]
    if (F > 0) {
        const int64_t total = n * F;
        for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = t / F;
            const int f = (int)(t - i * F);
            const int k = f / 3, c = f - 3 * k;
            sh[t] = ply_f32(rows + i * L.row_bytes, L.rest0 + 4 * (c * L.K + k));
        }
    }
}

extern "C" int32_t gsr_ply_unpack(const void* rows_dev, int64_t n, int32_t row_bytes, const int32_t* offsets, int32_t K, float* xyz, float* color,
                                  float* sh, float* opacity, float* scale, float* rot, float* cov6, int32_t device, void* stream) {
    if (n < 0 || K < 0 || K > 1024 || row_bytes <= 0 || !offsets ||
        (n > 0 && (!rows_dev || !xyz || !color || !opacity || !scale || !rot || !cov6 || (K > 0 && !sh))))
        return fail(GSR_E_INVALID, "gsr_ply_unpack: bad argument");
    GSR_TRY(open_device(device, "gsr_ply_unpack"));
    PlyLayout L;
    L.row_bytes = row_bytes; L.K = K;
    for (int i = 0; i < 3; ++i) { L.xyz[i] = offsets[i]; L.dc[i] = offsets[3 + i]; L.scale[i] = offsets[7 + i]; }
    L.opacity = offsets[6];
    for (int i = 0; i < 4; ++i) L.rot[i] = offsets[10 + i];
    L.rest0 = offsets[14];
    for (int i = 0; i < 15; ++i)       // in 64 bits: an offset near INT32_MAX plus its extent must not wrap and pass
        if (offsets[i] < 0 || (int64_t)offsets[i] + (i == 14 ? 12 * (int64_t)K : 4) > (int64_t)row_bytes) {
            if (i == 14 && K == 0) continue;
            return fail(GSR_E_INVALID, "gsr_ply_unpack: property offset %d outside the %d-byte row", offsets[i], row_bytes);
        }
    if (n == 0) return GSR_OK;
    hipLaunchKernelGGL(k_ply_unpack, dim3(stride_grid(n * (K > 0 ? 3 * K : 1))), dim3(256), 0, (hipStream_t)stream, n, (const unsigned char*)rows_dev, L, xyz, color, sh,
                       opacity, scale, rot, cov6);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

extern "C" int32_t gsr_decompose_cov(const float* cov6, int64_t n, int32_t mode, float* scaling, float* rotation, float* matrix,
                                     int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!cov6 || !scaling || !rotation))) return fail(GSR_E_INVALID, "gsr_decompose_cov: bad argument");
    if (mode != GSR_DECOMP_REFERENCE && mode != GSR_DECOMP_EXACT) return fail(GSR_E_INVALID, "gsr_decompose_cov: unknown mode %d", mode);
    GSR_TRY(open_device(device, "gsr_decompose_cov"));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_decompose_cov");
    const float* in = nullptr;
    float *sc = nullptr, *q = nullptr, *m = nullptr;
    GSR_TRY(os.in(cov6, (size_t)n * 24, &in));
    GSR_TRY(os.out(scaling, (size_t)n * 12, &sc));
    GSR_TRY(os.out(rotation, (size_t)n * 16, &q));
    GSR_TRY(os.out(matrix, (size_t)n * 36, &m));
    hipLaunchKernelGGL(k_decompose_cov, dim3(stride_grid(n)), dim3(256), 0, os.st, n, in, (int)mode, sc, q, m);
    return os.finish();
}
