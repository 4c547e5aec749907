/* gsr_test_hooks.h -- PRIVATE test hooks of libgsr_hip.so (not part of the drop-in boundary, include/gsr_hip.h).
 * They run the exact device functions the selection kernel uses on caller-supplied values, so that tests/ can pin
 * them against the host libm / the oracle.  Bound by tests through gaussiansplattingregistration_amd/_lib.py:TEST_HOOKS. */
#ifndef GSR_TEST_HOOKS_H
#define GSR_TEST_HOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* out[i] = the kernels' logf (glibc-compatible, gsr_math.h) of x[i]; host pointers. */
int32_t gsr_debug_logf(const float* x, int64_t n, float* out, int32_t device);
/* out[i] = KL gate value of child i against parent i as the selection kernel computes it; host pointers,
 * child_mean/parent_mean [n*3], child_cov6/parent_cov6 [n*6]. */
int32_t gsr_debug_kld(const float* child_mean, const float* child_cov6, const float* parent_mean,
                      const float* parent_cov6, int64_t n, float* out, int32_t device);
/* The KL gate decision of k_select for s2[i] = (smd + tr) - 3 and q = det_c[i] / det_p[i] against thr: reject[i] = the
 * kernel's decision (1 = KLD > thr), fast_log[i] = v_log_f32(det_c * (1 / det_p)) * ln 2, need_exact[i] = 1 where the decision
 * fell back to the IEEE division + glibc logf.  Host pointers. */
int32_t gsr_debug_kl_gate(const float* s2, const float* det_c, const float* det_p, int64_t n, float thr, uint8_t* reject,
                          float* fast_log, uint8_t* need_exact, int32_t device);
/* The stage-1 filter of k_select on n independent (parent, child) pairs, by the device functions the kernels use: the
 * "regular" predicate of both (is_regular), the parent's filter record (make_filter: white = filter certified, T1 = its bound,
 * clip_on = grid rows clipped to the ellipsoid) and reject[i] = 1 where stage 1 would drop the pair without the exact gates.
 * Host pointers; means [n*3], cov6 [n*6]. */
int32_t gsr_debug_stage1(const float* parent_mean, const float* parent_cov6, const float* child_mean, const float* child_cov6, int64_t n,
                         float kld_thr, uint8_t* parent_regular, uint8_t* child_regular, uint8_t* white, uint8_t* reject, float* T1,
                         uint8_t* clip_on, int32_t device);
/* The RANSAC sampler's raw draws (csrc/features.hip, formula in include/gsr_hip.h), on the host by the same __host__ __device__
 * function the kernels call: out[t * n + j] = row j of hypothesis k0 + t among m correspondences, before sorting. */
int32_t gsr_debug_ransac_sample(uint64_t seed, int64_t k0, int64_t count, int64_t m, int32_t n, int32_t* out);
/* The fixed-order float64 fold (csrc/gsr_fold.h) on x [n][3] (host): thread t of block b holds row 256 b + t, zeros past n;
 * block_fold_store<3, 4, order> (0: wave_sum_xor, 1: wave_sum_rows), then k_fold_partials<final_threads> (64 or 256) into out3. */
int32_t gsr_debug_fold(const double* x, int64_t n, int32_t order, int32_t final_threads, double* out3, int32_t device);
/* D[M x N] int32 = A[M x K] B[N x K]^T (int8, row-major, host) through the tile code of k_sc2_rows (csrc/sc2.hip): the operands are
 * copied into zero-padded device arrays of that kernel's layout and the kernel runs without its mask. */
int32_t gsr_test_i8_gemm_nt(const int8_t* A, int64_t M, const int8_t* B, int64_t N, int64_t K, int32_t* D, int32_t device);
/* gsr_sc2_correspondence on host arrays, leaving its stages in host arrays (any may be NULL): deg [m], seeds [n_seeds] (the
 * correspondence of every rank), rows [n_seeds * m] (masked second-order rows), k1 / k2 [n_seeds * 64] (selection order, -1 behind
 * the end), hyp [n_seeds * 12], good [n_seeds] (-1: invalid seed), rmse [n_seeds].  params / out: struct gsr_sc2_params / _result. */
int32_t gsr_test_sc2_stages(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                            const void* params, void* out, int32_t* deg, int32_t* seeds, int32_t* rows, int32_t* k1, int32_t* k2,
                            double* hyp, int32_t* good, double* rmse, int32_t device);
/* gsr_sc2_correspondence itself (arrays host or device as on_device says) with a timed stream event between its stages:
 * stage_ms[6] = gather + compatibility, seed sort, second-order rows (k_sc2_rows), consensus sets + hypotheses, scoring, refinement
 * (the host's reads between its steps included).  scripts/bench_sc2.py. */
int32_t gsr_test_sc2_timed(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                           const void* params, void* out, float* stage_ms, int32_t on_device, int32_t device, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* GSR_TEST_HOOKS_H */
