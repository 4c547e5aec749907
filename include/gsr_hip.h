/* include/gsr_hip.h -- C ABI of the MI355X (gfx950) registration backend, libgsr_hip.so.
 *
 * Drop-in boundary for the ONE data-parallel hot path of erikszasz/GaussianSplattingRegistration:
 * the Hierarchical-EM Gaussian-mixture downsampler and the per-iteration ICP step.  Plain pointers
 * and sizes only -- no torch, no C++ types.  Every entry point returns 0 on success or a negative
 * GSR_E_* code; gsr_last_error() returns the thread-local message of the last failure.
 *
 * Which reference interface each group replaces (paths relative to the reference repository):
 *
 *   gsr_hem_*   replaces the pybind11 module `mixture_bind` (src/cpp_ext/mixture_bind.cpp:11-61):
 *                 MixtureLevel.CreateMixtureLevel(xyz, colors, opacities, covariance, features)
 *                     src/cpp_ext/include/mixturelevel.hpp:17-22, src/mixturelevel.cpp:14-28  -> gsr_hem_set_level0
 *                 MixtureCreator.CreateMixture(clusterLevel, hemReduction, distanceDelta, colorDelta, decayRate, level)
 *                     src/cpp_ext/mixture_wrapper.hpp:10, mixture_wrapper.cpp:10-18              -> gsr_hem_create + gsr_hem_run_level x clusterLevel,
 *                                                                                                    or gsr_hem_run_levels (all levels in one call)
 *                 MixtureLevel.CreatePythonLists(level)  src/mixturelevel.cpp:30-70             -> gsr_hem_get_level
 *               (arithmetic: src/cpp_ext/src/mixture.cpp:54-64,66-285,287-333; include/gaussian.hpp:82-114;
 *                include/vec.hpp:736-768,863-872; src/pointindex.cpp:55-143; include/base.hpp:24-27,44-56)
 *
 *   gsr_icp_*   replaces what src/utils/local_registration_util.py:76-100 (do_icp_registration) reaches
 *               through open3d==0.16.0 (requirements.txt:3): registration_icp with
 *               TransformationEstimationPointToPoint / PointToPlane(loss) (:39-51, :58-73) and
 *               ICPConvergenceCriteria (:54-55).
 *
 *   gsr_normals_from_cov  replaces the estimate_normals() call on a cloud whose covariances were set
 *               from the splat covariances (src/utils/point_cloud_converter.py:40-43).
 *
 * Memory: every array argument is row-major and contiguous.  `on_device != 0` means the pointer is a
 * HIP device pointer on the context's device (e.g. a PyTorch-ROCm tensor's data_ptr()); otherwise it
 * is host memory and the library stages it.  The caller owns everything it passes and receives; the
 * library owns only its context and workspace, released by the matching *_destroy.
 * Contexts are single-owner and not re-entrant; different contexts may run concurrently on
 * different streams / GPUs.  `stream` is a hipStream_t (NULL = the default stream).
 */
#ifndef GSR_HIP_H
#define GSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK              0
#define GSR_E_INVALID      -1   /* bad argument (NULL handle, negative size, wrong state) */
#define GSR_E_HIP          -2   /* a HIP runtime call failed (message carries hipGetErrorString) */
#define GSR_E_NO_DEVICE    -3   /* no gfx950 device visible: the product path has no CPU fallback */
#define GSR_E_PRECONDITION -4   /* ICP preconditions: max_corr <= 0, point-to-plane without normals, empty cloud */

const char* gsr_last_error(void);
/* "gsr_hip <version> gfx950" */
const char* gsr_version(void);
/* Number of visible HIP devices (0 when none; never fails). */
int32_t gsr_device_count(void);

/* ------------------------------------------------------------------------------------ communicator */

/* Multi-GPU runs (BASELINE configs 4 and 5; the reference has no distributed code): one process per GPU,
 * RCCL over xGMI called FROM THE LIBRARY on the context's own stream -- nothing crosses into the host language per ICP
 * iteration or per HEM level.  Rank 0 calls gsr_comm_get_unique_id and hands the GSR_COMM_ID_BYTES bytes to every rank by any
 * means (the Python side broadcasts them with torch.distributed); every rank then calls gsr_comm_create (ncclCommInitRank:
 * collective, blocks until all ranks have called it).  librccl.so.1 is opened lazily: a single-GPU user never loads it.
 * gsr_comm_create_callbacks builds the same object over host-language collectives on DEVICE buffers (test boxes where two
 * ranks share one GPU, which RCCL refuses): a callback is called after the library has synchronised the stream and must have
 * completed when it returns 0. */
typedef struct gsr_comm gsr_comm;
#define GSR_COMM_ID_BYTES 128
#define GSR_DT_F64 0
#define GSR_DT_F32 1
#define GSR_DT_I32 2
#define GSR_DT_U32 3
#define GSR_DT_U64 4
#define GSR_OP_SUM 0
#define GSR_OP_MAX 1
typedef struct gsr_comm_callbacks {
    /* replace dev_buf[count] (elements of GSR_DT_*) by its element-wise GSR_OP_* over the ranks */
    int32_t (*allreduce)(void* dev_buf, int64_t count, int32_t dtype, int32_t op, void* user);
    /* dev_recv[r * bytes_per_rank ...] = rank r's dev_send[0 .. bytes_per_rank) */
    int32_t (*allgather)(const void* dev_send, void* dev_recv, int64_t bytes_per_rank, void* user);
    /* personalised exchange: send_bytes[r] bytes at dev_send + send_off[r] go to rank r, which receives them at its
     * dev_recv + recv_off[this rank]; the arrays have one entry per rank (the entry of the calling rank is handled by the library) */
    int32_t (*exchange)(const void* dev_send, const int64_t* send_off, const int64_t* send_bytes, void* dev_recv,
                        const int64_t* recv_off, const int64_t* recv_bytes, void* user);
    void* user;
} gsr_comm_callbacks;
int32_t gsr_comm_get_unique_id(void* id128);
int32_t gsr_comm_create(gsr_comm** out, const void* id128, int32_t rank, int32_t world, int32_t device);
int32_t gsr_comm_create_callbacks(gsr_comm** out, int32_t rank, int32_t world, int32_t device, const gsr_comm_callbacks* cb);
int32_t gsr_comm_destroy(gsr_comm* comm);
int32_t gsr_comm_rank(const gsr_comm* comm);
int32_t gsr_comm_world(const gsr_comm* comm);
/* The operations themselves (device buffers, enqueued on `stream` with the RCCL transport); exposed for tests and for host code
 * that shares the communicator. */
int32_t gsr_comm_allreduce(gsr_comm* comm, void* dev_buf, int64_t count, int32_t dtype, int32_t op, void* stream);
int32_t gsr_comm_allgather(gsr_comm* comm, const void* dev_send, void* dev_recv, int64_t bytes_per_rank, void* stream);
int32_t gsr_comm_exchange(gsr_comm* comm, const void* dev_send, const int64_t* send_off, const int64_t* send_bytes, void* dev_recv,
                          const int64_t* recv_off, const int64_t* recv_bytes, void* stream);

/* ------------------------------------------------------------------------------------------- HEM */

typedef struct gsr_hem_ctx gsr_hem_ctx;

/* RNG that draws the parent flags (mixture.cpp:256-259,330):
 *   GSR_RNG_GLIBC  glibc TYPE_3 rand() model, eight rand()%16 nibbles per flag (base.hpp:44-56);
 *                  seed 1 + skip 0 replays a fresh reference process.  Parity mode (default).
 *   GSR_RNG_HASH   counter-based hash of (seed, draw index): same distribution, not the same stream. */
#define GSR_RNG_GLIBC 0
#define GSR_RNG_HASH  1

int32_t gsr_hem_create(gsr_hem_ctx** out, int32_t device, void* stream);
int32_t gsr_hem_destroy(gsr_hem_ctx* ctx);

/* hemReduction, distanceDelta, colorDelta, decayRate -- src/params/merge_parameters.py:5-10 */
int32_t gsr_hem_set_params(gsr_hem_ctx* ctx, float hem_reduction, float distance_delta,
                           float color_delta, float decay_rate);
/* rng_skip = number of hem::rand() values already consumed from the stream (lets a second cloud
 * continue the first cloud's stream as qt_gaussian_mixture.py:55,79 does). */
int32_t gsr_hem_set_rng(gsr_hem_ctx* ctx, int32_t mode, uint32_t seed, uint64_t rng_skip);
int32_t gsr_hem_get_rng_position(gsr_hem_ctx* ctx, uint64_t* draws);

/* Level 0: xyz[n*3], color[n*3] (SH DC), cov6[n*6] (xx,xy,xz,yy,yz,zz), opacity[n] (RAW logit),
 * sh[n*F] (SH rest, coefficient-major); float32.  Sets weight = 1 and draws the n initial parent
 * flags (Mixture::initMixture, mixture.cpp:287-333).  F may be 0 (sh may then be NULL).
 * on_device: 0 = host arrays (copied), 1 = device arrays (copied), 2 = device arrays BORROWED without a copy: they must
 * stay valid and unchanged until the next gsr_hem_run_level (or gsr_hem_set_level0 / destroy) returns. */
int32_t gsr_hem_set_level0(gsr_hem_ctx* ctx, const float* xyz, const float* color, const float* cov6,
                           const float* opacity, const float* sh, int64_t n, int32_t F, int32_t on_device);
/* Override internal per-component state of the CURRENT level (either may be NULL):
 * parent_mask[n] (0/1 bytes, consumes no RNG draws) and weight[n].  Host pointers. */
int32_t gsr_hem_set_state(gsr_hem_ctx* ctx, const uint8_t* parent_mask, const float* weight);

/* Work-sharded levels for ONE large cloud on several GPUs (the reference has no such
 * thing).  Every rank holds the full level (replicated data, deterministic replicated grid); rank r of
 * `world` evaluates the contiguous run [P r/world, P (r+1)/world) of the cell-sorted parents -- a spatial
 * slab -- and the level makes two exchanges:
 *   allreduce(dev_f32, count, user)   the per-child sums of wL: replace the float32 DEVICE buffer (n values) by its
 *                                     element-wise sum over the ranks (RCCL all-reduce in the host language);
 *   allgather(send, recv, bytes, user) the merged components: every rank contributes `bytes` bytes at `send` (device),
 *                                     `recv` (device, world * bytes) receives rank r's contribution at offset r * bytes.
 * Both must have completed (or be ordered on the context's stream) when they return 0.
 * world == 1 / NULL callbacks restore the single-GPU level. */
typedef int32_t (*gsr_allreduce_dev_fn)(void* dev_f32, int64_t count, void* user);
typedef int32_t (*gsr_allgather_dev_fn)(const void* dev_send, void* dev_recv, int64_t bytes_per_rank, void* user);
int32_t gsr_hem_set_shard(gsr_hem_ctx* ctx, int32_t rank, int32_t world, gsr_allreduce_dev_fn allreduce,
                          gsr_allgather_dev_fn allgather, void* user);

/* SPATIALLY PARTITIONED levels for one large cloud on several GPUs (BASELINE config 5; the reference has no
 * such thing).  Every rank owns a subset of the cloud -- compact blocks keep the halo small (parallel.block_of), but any disjoint
 * cover works -- and passes its components with their GLOBAL indices (ascending) to gsr_hem_set_level0_part; gsr_hem_run_level
 * then runs the level on owned + ghost components and the result is BIT FOR BIT the single-GPU level, distributed: per level
 *   - integer all-reduces of the bounding box (24 bytes), the axis histograms (12 KB) and two bit maps over the level's global
 *     indices (n_global / 4 bytes): every rank derives the same grid and the same global output ranks;
 *   - one all-gather of two bit masks over the grid's cells (which cells can my parents take regular / irregular candidates from:
 *     the box of the pre-reject ellipsoid / of the search sphere) and the personalised exchange of the halo, in two messages per
 *     neighbour along the same lists: 72-byte rows {packed record, global index, index at the owner} on the context's stream, and
 *     the 4F-byte SH rows -- which only the M-step reads -- on a second stream, overlapped with the grid phase and the selection;
 *   - five small exchanges along the same halo lists for the per-child sums: maxima (u32), the owners' maxima back, 64-bit
 *     fixed-point partial sums, the owners' float32 sums back -- no floating-point value is ever combined across ranks.
 * The new level stays distributed (gsr_hem_get_level returns the owned rows, gsr_hem_get_gids their global indices; ownership
 * follows the parents).  All of it goes through the communicator: RCCL enqueued on the context's stream, or callbacks.
 * A level's rank-local PRECONDITIONS (a rank that owns nothing, 2^30 components, more than 8 ranks) are agreed on with one all-reduce
 * of a status word before its first data collective: every rank returns the same error.  Beyond that ERRORS ARE LOCAL: a rank whose
 * call fails (an allocation, a callback returning non-zero) returns its error code while the
 * other ranks are inside or in front of the next collective -- as with any RCCL program the caller must then abort the process
 * group (ncclCommAbort / tear the job down); the library does not try to agree on a status across ranks.  The same holds for
 * gsr_icp_register with a communicator or an all-reduce callback. */
int32_t gsr_hem_set_comm(gsr_hem_ctx* ctx, gsr_comm* comm);
int32_t gsr_hem_set_level0_part(gsr_hem_ctx* ctx, const float* xyz, const float* color, const float* cov6, const float* opacity,
                                const float* sh, const uint32_t* gid, int64_t n_own, int64_t n_global, int32_t F, int32_t on_device);
int32_t gsr_hem_get_gids(gsr_hem_ctx* ctx, uint32_t* gid, int32_t on_device);
/* of the most recent partitioned level: [0] ghost components received  [1] halo rows sent  [2] bytes received in the halo exchange
 * [3] bytes received in the five sum exchanges  [4] parents of the level over all ranks  [5] orphans over all ranks
 * [6] components erased over all ranks  [7] components of the CURRENT level over all ranks */
int32_t gsr_hem_get_part_stats(gsr_hem_ctx* ctx, int64_t* out8);
/* durations (ms, device events) of the most recent partitioned level's halo exchanges: [0] the 72-byte rows (on the critical path)
 * [1] the SH rows (second stream, overlapped)  [2], [3] reserved */
int32_t gsr_hem_get_part_ms(gsr_hem_ctx* ctx, float* out4);

/* Zero-copy level output ("returning torch tensors, zero-copy on device"): the NEXT gsr_hem_run_level writes its level
 * straight into these caller-owned DEVICE arrays -- xyz[rows*3], color[rows*3], cov6[rows*6], opacity[rows], sh[rows*F] (sh may be
 * NULL when F = 0) -- instead of the context's own buffers, and that memory then IS the current level (borrowed exactly like an
 * on_device = 2 level 0): nothing is copied on the way out, nothing on the way into the level after.  capacity_rows >= the size of
 * the level being reduced is always enough (a level never grows); the call fails cleanly if the new level does not fit.  The
 * arrays hold the level when run_level returns (n_out rows) and must stay valid and unchanged until the run_level AFTER that one
 * (or gsr_hem_set_level0 / destroy) has returned.  One request covers one level; capacity_rows <= 0 withdraws it.
 * (The reference copies every level by value, mixture.cpp:342, and then into Python lists, mixturelevel.cpp:30-70.) */
int32_t gsr_hem_set_output(gsr_hem_ctx* ctx, float* xyz, float* color, float* cov6, float* opacity, float* sh, int64_t capacity_rows);

/* One clustering level on the current level (Mixture::createClusterLevel, mixture.cpp:66-285).
 * n_out = components of the new level (after the validity erase); n_dropped = components erased by
 * it (the reference prints these to cerr, mixture.cpp:270-274).  The new level becomes current.
 * The call returns when the level is complete.  On one GPU it makes ONE host round trip, behind the level's last kernel (the level's
 * own prologue -- grid geometry, parent count -- was computed with its input and travelled with the round trip of gsr_hem_set_level0 /
 * of the level before; every other count stays on the device and every write is clamped to the context's buffers).  When those buffers
 * turn out too small -- a context's first level, a much larger cloud than before -- the level is run again with every buffer sized from
 * counts read back on the way (gsr_hem_get_stats_ex [6], [7]); its input is never written, the result is the same.  GSR_HEM_ASYNC=0
 * always takes that second schedule.  (The reference's level has no such boundary: one function, mixture.cpp:25-35.) */
int32_t gsr_hem_run_level(gsr_hem_ctx* ctx, int64_t* n_out, int64_t* n_dropped);

/* MixtureCreator::CreateMixture(clusterLevel, ...) in ONE call (mixture_wrapper.cpp:10-18: the reference runs every level inside one
 * function and returns the list of levels): `n_levels` clustering levels on the current level, each written straight into caller-owned
 * DEVICE arenas -- xyz[arena_rows*3], color[arena_rows*3], cov6[arena_rows*6], opacity[arena_rows], sh[arena_rows*F] (NULL when
 * F = 0) -- one level behind the other: level k occupies rows [reports[k].offset_rows, + reports[k].rows) of every arena (offsets are
 * multiples of 64 rows, so every level's arrays start 256-byte aligned).  A level needs room for as many rows as its INPUT has while it
 * runs: the call fails cleanly (GSR_E_INVALID, nothing of that level written) when offset + input rows > arena_rows; arena_rows =
 * n_levels x (rows of level 0) always suffices; 1.5 x is enough for a reduction by 3 per level, a cloud of discs and needles (levels keep 60 - 90 % of their input) needs 1.7 x for three levels.  Equivalent to gsr_hem_set_output +
 * gsr_hem_run_level per level -- the same bits -- without a return to the host language between the levels (a Python caller spent
 * ~0.15 ms per level there, a tenth of a 556 k-splat level); reports[k] carries what gsr_hem_get_stats / _stats_ex / _phase_ms /
 * _kernel_ms / _rng_position would have returned after level k.
 * normals (optional, DEVICE, arena_rows*3 float64): the normal of every component of every new level -- the eigenvector of the smallest
 * eigenvalue of its covariance, what `estimate_normals()` gives a cloud whose covariances are set (point_cloud_converter.py:40-43),
 * bit for bit gsr_normals_from_cov -- at the level's row offset: the normals leave with the level, computed
 * on a side stream beside the next level and joined into the context's stream before the call returns.
 * normals0 (optional, DEVICE, rows of the current level * 3 float64): the same for the level the call starts from.
 * The arenas must stay valid and unchanged until the next gsr_hem_run_level(s) / gsr_hem_set_level0 / destroy has returned (the last
 * level of the call is the context's current level, borrowed).  Not for partitioned / sharded levels (gsr_hem_set_comm, _set_shard). */
typedef struct gsr_hem_level_report {
    int64_t offset_rows;        /* first row of the level in the arenas */
    int64_t rows;               /* components of the level (after the validity erase) */
    int64_t dropped;            /* components the validity erase removed */
    uint64_t rng_position;      /* gsr_hem_get_rng_position after the level */
    int64_t stats[8];           /* gsr_hem_get_stats */
    int64_t stats_ex[8];        /* gsr_hem_get_stats_ex */
    float phase_ms[8];          /* gsr_hem_get_phase_ms */
    float kernel_ms[8];         /* gsr_hem_get_kernel_ms */
} gsr_hem_level_report;
int32_t gsr_hem_run_levels(gsr_hem_ctx* ctx, int32_t n_levels, float* xyz, float* color, float* cov6, float* opacity, float* sh,
                           double* normals, double* normals0, int64_t arena_rows,
                           gsr_hem_level_report* reports);

int32_t gsr_hem_level_size(gsr_hem_ctx* ctx, int64_t* n, int32_t* F);
/* Copy the current level into caller buffers (any may be NULL).  weight / is_parent are internal
 * state the reference never exports (mixture.hpp:33-44); offered for single-level checks. */
int32_t gsr_hem_get_level(gsr_hem_ctx* ctx, float* xyz, float* color, float* cov6, float* opacity,
                          float* sh, float* weight, uint8_t* is_parent, int32_t on_device);

/* Counters of the most recent gsr_hem_run_level:
 *  [0] parents  [1] accepted (parent,child) pairs  [2] orphans  [3] dropped  [4] candidates scanned
 *  [5] grid cells  [6] components in  [7] components out */
int32_t gsr_hem_get_stats(gsr_hem_ctx* ctx, int64_t* out8);
/* More counters of the most recent level:  [0] components outside the stage-1 filter's precondition ("irregular": not
 * verified symmetric positive definite with an accurate float32 determinant -- they take the exact gates only)
 * [1] 1 = the one-pass selection ran, 0 = the COUNT + FILL fallback  [2] 1 = a bucket region of the pair partition overflowed (in this level or an
 * earlier one of the context) and the level's sums took the exact partition  [3] heavy parents (candidates scanned > 16 x the mean: cut
 * into work items)  [4] their work items  [5] the largest number of accepted pairs of one parent
 * [6] host round trips of the level (1: the asynchronous schedule; 4-6: the synchronous one)
 * [7] schedule: 1 = no round trip between the level's first and last kernel, 0 = synchronous (buffers sized from counts read back on the way: a
 *     context's first level, partitioned / sharded levels, GSR_HEM_ASYNC=0), 2 = an asynchronous attempt whose buffers were too small, rerun. */
int32_t gsr_hem_get_stats_ex(gsr_hem_ctx* ctx, int64_t* out8);
/* Device time of the phases of the most recent level, in milliseconds (hipEvent pairs on the
 * context's stream):  [0] prep+grid  [1] selection (count+scan+fill)  [2] per-child sums
 * [3] M-step + orphans  [4] flags+validity  [5] whole level
 * [6] the k_select<COUNT> launch alone (two-pass fallback only, else 0)
 * [7] the k_select<SPARSE> launch alone (or k_select<FILL> on the fallback) */
int32_t gsr_hem_get_phase_ms(gsr_hem_ctx* ctx, float* out8);
/* Device time of single kernel launches of the most recent level (hipEvent pairs on the context's stream), milliseconds:
 *  [0] k_select (the light parents' launch; the heavy work items run beside it)  [1] k_mstep  [2] k_partition  [3] k_bucket_sum
 *  [4..7] reserved (0).  What bench.py prices against the roofline. */
int32_t gsr_hem_get_kernel_ms(gsr_hem_ctx* ctx, float* out8);
/* How much of the above a level records (the reference has no counterpart: its only trace is a `cout` per level, mixture.cpp:32).
 * An event between two kernels is a packet of its own on the stream -- 22 per level, 0.1 ms of a 5 M-splat level, 6 % of a 556 k one:
 *   0  nothing (every figure of gsr_hem_get_phase_ms / _kernel_ms reads 0)
 *   1  the whole level and the launches of k_select and k_mstep: phase [5] [6] [7], kernel [0] [1]   (the default)
 *   2  every phase and kernel listed above
 * The environment variable GSR_HEM_TIMING sets the value a new context starts with. */
int32_t gsr_hem_set_timing(gsr_hem_ctx* ctx, int32_t level);

/* ------------------------------------------------------------------------------------------- ICP */

typedef struct gsr_icp_ctx gsr_icp_ctx;

#define GSR_ICP_POINT_TO_POINT 0   /* LocalRegistrationType.ICP_Point_To_Point, local_registration_util.py:33 */
#define GSR_ICP_POINT_TO_PLANE 1   /* LocalRegistrationType.ICP_Point_To_Plane, :34 */
#define GSR_ICP_GENERALIZED    2   /* LocalRegistrationType.ICP_General, :36 (registration_generalized_icp, :96-98) */
#define GSR_ICP_COLORED        3   /* LocalRegistrationType.ICP_Color, :35 (registration_colored_icp, :92-94) */
/* TransformationEstimationPointToPoint(with_scaling=True), i.e. Eigen::umeyama(src, dst, true): the update is a SIMILARITY
 * [c R | t] and so is the registration's transform (two splat scenes from separate structure-from-motion runs share no unit of
 * length).  The value is the point-to-point kind with the GSR_ICP_WITH_SCALING bit; that bit on any other kind (5, 6, 7) is
 * GSR_E_INVALID with a message -- Open3D offers scaling for point-to-point only -- and so is the scaled kind with a loss other than
 * GSR_LOSS_L2 (kind 0 ignores the loss argument).  Fitness, RMSE and max_corr are measured in the target's frame after T, as for
 * every kind.  Where Eigen would divide by zero (one correspondence, coincident source points: var = 0 or c = 0) the update is
 * the identity.  Open3D is absent from the test machines: like the rest of the ICP half this is checked against a float64
 * restatement of the definition (tests/sim3_model.py), parity with Open3D itself is unpinned. */
#define GSR_ICP_WITH_SCALING   4
#define GSR_ICP_POINT_TO_POINT_SCALED (GSR_ICP_POINT_TO_POINT | GSR_ICP_WITH_SCALING)   /* = 4 */

#define GSR_LOSS_L2     0          /* KernelLossFunctionType.Loss_None or k == 0, :63-64 */
#define GSR_LOSS_TUKEY  1
#define GSR_LOSS_CAUCHY 2
#define GSR_LOSS_GM     3
#define GSR_LOSS_HUBER  4

int32_t gsr_icp_create(gsr_icp_ctx** out, int32_t device, void* stream);
int32_t gsr_icp_destroy(gsr_icp_ctx* ctx);

/* Target cloud: xyz[n*3] float32 (the reference widens the float32 splat positions to float64,
 * point_cloud_converter.py:33), normals[n*3] float64 or NULL (Open3D normals are float64).  Builds
 * the uniform-grid index used for the exact nearest-neighbour search (expanding rings of cells, at
 * most ceil(max_corr / cell) of them).  Call it BEFORE gsr_icp_set_source: the source is kept sorted by
 * this grid, and a new target invalidates the source. */
int32_t gsr_icp_set_target(gsr_icp_ctx* ctx, const float* xyz, const double* normals, int64_t n,
                           double max_corr, int32_t on_device);
int32_t gsr_icp_set_source(gsr_icp_ctx* ctx, const float* xyz, int64_t n, int32_t on_device);
/* Per-point covariances for GSR_ICP_GENERALIZED: cov6[n*6] float64 (xx, xy, xz, yy, yz, zz), in the order of the
 * points last given to gsr_icp_set_target / gsr_icp_set_source (call these after them).  The reference's clouds
 * carry the splats' own covariances (point_cloud_converter.py:38), which Open3D's generalized ICP then uses as
 * they are; the source covariances follow the source under the current transform (C <- R C R^T). */
int32_t gsr_icp_set_target_cov(gsr_icp_ctx* ctx, const double* cov6, int32_t on_device);
int32_t gsr_icp_set_source_cov(gsr_icp_ctx* ctx, const double* cov6, int32_t on_device);
/* Colours for GSR_ICP_COLORED: rgb[n*3] float64 in the order of the points last given to gsr_icp_set_target /
 * gsr_icp_set_source (call after them; the target needs normals).  The target call also prepares the cloud as Open3D's
 * InitializePointCloudForColoredICP does: per point, the 30 nearest neighbours within 2 * max_corr (ordered by
 * distance, then index), a least-squares colour gradient in the tangent plane.  lambda_geometric defaults to 0.968
 * (TransformationEstimationForColoredICP).  gsr_icp_get_color_gradient: the gradients [n*3], host memory, caller order. */
int32_t gsr_icp_set_target_color(gsr_icp_ctx* ctx, const double* rgb, int32_t on_device);
int32_t gsr_icp_set_source_color(gsr_icp_ctx* ctx, const double* rgb, int32_t on_device);
int32_t gsr_icp_set_lambda_geometric(gsr_icp_ctx* ctx, double lambda_geometric);
int32_t gsr_icp_get_color_gradient(gsr_icp_ctx* ctx, double* out);
/* Multi-GPU source split: this rank owns source points, the target is replicated.  `allreduce` is
 * called once per correspondence evaluation with the rank-local accumulator vector (float64[len],
 * host memory) and must replace it by the element-wise sum over ranks (RCCL/gloo all-reduce in the
 * host language).  NULL = single rank.  n_source_global = source points over all ranks. */
typedef int32_t (*gsr_allreduce_fn)(double* buf, int32_t len, void* user);
int32_t gsr_icp_set_allreduce(gsr_icp_ctx* ctx, gsr_allreduce_fn fn, void* user, int64_t n_source_global);
/* The same with a DEVICE buffer: `fn(dev_f64, count, user)` must replace the float64 device vector by its sum over the
 * ranks, ordered on the context's stream (an RCCL all-reduce enqueued on that stream, or a synchronous one).  The
 * iteration loop then stays device resident: per iteration one reduction kernel, the collective on 32 doubles, one
 * kernel that tests convergence and solves on EVERY rank from the identical reduced vector.  A rank may hold an empty
 * shard (gsr_icp_set_source with n = 0).  Installing one kind of callback removes the other; NULL restores single-GPU. */
typedef int32_t (*gsr_allreduce_dev64_fn)(void* dev_f64, int64_t count, void* user);
int32_t gsr_icp_set_allreduce_dev(gsr_icp_ctx* ctx, gsr_allreduce_dev64_fn fn, void* user, int64_t n_source_global);
/* The same through a communicator: per iteration the accumulate kernel (its last workgroup folds the block partials), ONE
 * all-reduce of 32 float64 enqueued on the context's stream (ncclAllReduce with the RCCL transport: no host involvement), and
 * the solve kernel.  comm = NULL restores single-GPU.  The communicator must outlive the context's use of it. */
int32_t gsr_icp_set_comm(gsr_icp_ctx* ctx, gsr_comm* comm, int64_t n_source_global);

/* One correspondence evaluation + accumulator reduction at transform T (row-major 4x4 float64):
 * acc[0]=count, acc[1]=sum d^2, then for point-to-point acc[2..4]=sum p, [5..7]=sum q, [8..16]=sum p q^T
 * (p = transformed source, q = matched target, both relative to the target-bbox centre); the scaled point-to-point kind has the
 * same seventeen and acc[17]=sum |p|^2;
 * for point-to-plane and generalized ICP acc[2..22]=upper triangle of J^T w J (row-major), [23..28]=J^T w r,
 * [29]=sum r^2 (generalized: three residual rows per pair, J = W [-skew(p) | I], W = (Ct + R Cs R^T)^-1/2;
 * colored: a geometric and a photometric row per pair).
 * len(acc) = GSR_ICP_ACC_LEN.  This is the "hot loop" exposed for tests and for RCCL all-reduce. */
#define GSR_ICP_ACC_LEN 32
int32_t gsr_icp_accumulate(gsr_icp_ctx* ctx, const double* T, int32_t kind, int32_t loss, double k,
                           double* acc);

/* registration_icp: iterate until |dfitness| < rel_fitness && |drmse| < rel_rmse or max_iter.
 * out_T row-major 4x4 float64.  iterations = estimator updates applied. */
int32_t gsr_icp_register(gsr_icp_ctx* ctx, const double* init_T, int32_t kind, int32_t loss, double k,
                         double rel_fitness, double rel_rmse, int32_t max_iter,
                         double* out_T, double* fitness, double* inlier_rmse, int32_t* iterations);
/* The same with the two CLOUDS as arguments -- Open3D's own signature, registration_icp(source, target, max_correspondence_distance,
 * init, estimation_method, criteria) (local_registration_util.py:88-90): gsr_icp_set_target + gsr_icp_set_source + gsr_icp_register in
 * one call, without a return to the host language or a stream synchronisation between them; same result, bit for bit.  Point-to-point
 * (plain or scaled) and point-to-plane (tgt_normals[nt*3] float64, required for the latter; ignored for the former); one process, one GPU (an installed
 * communicator / all-reduce callback is removed).  on_device: 0 = host arrays, 1 = device arrays (read in place). */
int32_t gsr_icp_register_clouds(gsr_icp_ctx* ctx, const float* src_xyz, int64_t ns, const float* tgt_xyz, const double* tgt_normals,
                                int64_t nt, int32_t on_device, double max_corr, const double* init_T, int32_t kind, int32_t loss,
                                double k, double rel_fitness, double rel_rmse, int32_t max_iter, double* out_T, double* fitness,
                                double* inlier_rmse, int32_t* iterations);
/* The coarse-to-fine schedule in one call (MultiScaleRegistratorMixture._register_main_point_clouds, qt_multiscale_registrator.py:197-236: entry k registers
 * the k-th coarsest level of the two clouds, starting from the transform entry k - 1 ended with): gsr_icp_register_clouds per entry without a return to
 * the host language between the entries.  entries[] coarsest first; results[k] = entry k's outcome (its start, its transform, fitness, RMSE, iterations, the
 * device milliseconds of its index build and of its iterations); out_T = the last entry's transform (init_T when n_entries = 0). */
typedef struct gsr_icp_entry {
    const float* src_xyz; int64_t ns;
    const float* tgt_xyz; const double* tgt_normals; int64_t nt;
    double max_corr;            /* max_correspondence_distance of the entry */
    int32_t max_iter; int32_t reserved;
} gsr_icp_entry;
typedef struct gsr_icp_entry_result {
    double init_T[16], T[16];
    double fitness, inlier_rmse;
    int32_t iterations, evaluations;
    float ms_build, ms_iters;
} gsr_icp_entry_result;
int32_t gsr_icp_register_multiscale(gsr_icp_ctx* ctx, int32_t n_entries, const gsr_icp_entry* entries, int32_t on_device, const double* init_T,
                                    int32_t kind, int32_t loss, double k, double rel_fitness, double rel_rmse, gsr_icp_entry_result* results,
                                    double* out_T);
/* Nearest target index (or -1) and squared distance for every source point at transform T. */
int32_t gsr_icp_correspondences(gsr_icp_ctx* ctx, const double* T, int64_t* idx, double* d2);
/* Information matrix of the pair at transform T (Open3D's get_information_matrix_from_point_clouds): every source point is moved by T,
 * its correspondence is its nearest target point q with |T p - q|^2 < max_corr^2 (strict; the context's max_corr, the search of an
 * evaluation), and info36 = sum over the correspondences of G^T G with G = [ -[q]x | I3 ] at the TARGET point -- rotation columns
 * first, row-major 6x6 float64 on the host; info36[35] = *n_corr = the number of correspondences (n_corr may be NULL).  No
 * correspondence: the zero matrix and 0, not an error.  One kernel of ten float64 sums per lane (n, sum q, sum q q^T) and the
 * fixed-order reduction of gsr_icp_accumulate: the same inputs give the same bits.  One process, one GPU: a context with a communicator
 * or an all-reduce callback installed is GSR_E_INVALID. */
int32_t gsr_icp_information(gsr_icp_ctx* ctx, const double* T, double* info36, int64_t* n_corr);
/* Device milliseconds: [0] target index build, [1] all correspondence/accumulate kernels of the last
 * gsr_icp_register, [2] their count. */
int32_t gsr_icp_get_timing(gsr_icp_ctx* ctx, float* out3);

/* Normals = unit eigenvector of the smallest eigenvalue of each 3x3 splat covariance, computed in
 * float64 from the float32 covariance widened to float64 (as Open3D does on the converted cloud);
 * a zero vector becomes (0,0,1), and so does the normal of a covariance with a NaN or infinite entry.
 * cov6[n*6] float32 in, normals[n*3] float64 out. */
int32_t gsr_normals_from_cov(const float* cov6, int64_t n, double* normals, int32_t on_device,
                             int32_t device, void* stream);

/* Estimator solve on the HOST from a reduced accumulator vector (no GPU involved): the 3x3 Jacobi
 * SVD of Eigen::umeyama (point-to-point, plain or scaled) or the 6x6 LDL^T solve + Rz*Ry*Rx of Open3D's point-to-plane
 * estimator.  centre[3] = the point the point-to-point sums are relative to (ignored for
 * point-to-plane).  update = row-major 4x4.  Every rank of a multi-GPU run calls this on the same
 * all-reduced vector and so gets the identical update. */
int32_t gsr_icp_solve(const double* acc, int32_t kind, const double* centre, double* update);
/* The centre used by the context's point-to-point sums (target bounding-box centre). */
int32_t gsr_icp_get_centre(gsr_icp_ctx* ctx, double* centre3);

/* Normals of a cloud that has NO covariances -- a sparse (COLMAP) input cloud of the multiscale worker's sparse
 * pre-registration (src/gui/workers/registration/qt_multiscale_registrator.py:74-90, src/utils/file_loader.py:20-30):
 * replaces the estimate_normals() call of convert_input_pc_to_open3d_pc (src/utils/point_cloud_converter.py:9-28), i.e.
 * Open3D's default KDTreeSearchParamKNN(knn = 30) + covariance of the neighbourhood + FastEigen3x3.
 * xyz[n*3] float32, normals[n*3] float64 (host or device as on_device says), knn in [1, 30]. */
int32_t gsr_normals_knn(const float* xyz, int64_t n, int32_t knn, double* normals, int32_t on_device, int32_t device, void* stream);

/* Covariances for generalized ICP on a cloud that carries none: Open3D's InitializePointCloudForGeneralizedICP
 * (GeneralizedICP.cpp) -- C_i = Rx diag(epsilon, 1, 1) Rx^T, Rx = the rotation taking e1 to the point's normal.  The reference
 * reaches it through registration_generalized_icp on its SPARSE input clouds (local_registration_util.py:96-98 called from
 * qt_multiscale_registrator.py:82-85), which have KNN-30 normals (point_cloud_converter.py:26) and no covariances; a cloud
 * without normals gets gsr_normals_knn(knn = 20) first, as Open3D does.  epsilon = 1e-3 is Open3D's default.
 * normals[n*3] float64 in, cov6[n*6] float64 (xx, xy, xz, yy, yz, zz) out; host or device as on_device says. */
int32_t gsr_cov_from_normals(const double* normals, int64_t n, double epsilon, double* cov6, int32_t on_device,
                             int32_t device, void* stream);

/* ------------------------------------------------------------------------------------ level export */

/* Scaling / rotation of every component from its covariance, on the device: replaces
 * GaussianModel.decompose_covariance_matrix + matrices_to_quaternions, which GaussianModel.from_mixture runs on every
 * HEM level (src/models/gaussian_model.py:141-153,242-265; src/utils/general_utils.py:94-100).
 *   GSR_DECOMP_REFERENCE  the reference's arithmetic, bug for bug: scaling[k] = the eigenVALUE whose eigenvector is most
 *                         aligned with axis k (0 if none claims it, the larger eigenvalue if two do), rotation = the
 *                         trace-formula quaternion (w, x, y, z) of the matrix whose row k is the claiming ROW of eigh's
 *                         eigenvector matrix (csrc/model.hip spells it out).
 *   GSR_DECOMP_EXACT      scaling = log standard deviations, rotation = unit quaternion of a proper rotation, such that
 *                         R diag(exp(scaling))^2 R^T reproduces the covariance (what save_ply of a level needs).
 *                         Eigenvalues are clamped at 1e-30; a covariance with a NaN or infinite entry leaves as NaN in
 *                         scaling, rotation and matrix.
 * cov6[n*6] (xx,xy,xz,yy,yz,zz), scaling[n*3], rotation[n*4], matrix[n*9] or NULL (the 3x3 the quaternion was taken from,
 * row-major); float32, all host or all device as on_device says. */
#define GSR_DECOMP_REFERENCE 0
#define GSR_DECOMP_EXACT     1
int32_t gsr_decompose_cov(const float* cov6, int64_t n, int32_t mode, float* scaling, float* rotation, float* matrix,
                          int32_t on_device, int32_t device, void* stream);

/* The other direction, and its derivative (csrc/covgrad.hip, csrc/gsr_covbuild.h): the covariance of every splat from its
 * log-scales and RAW quaternion (w, x, y, z; any norm but 0), cov = R(q / |q|) diag(exp(scaling))^2 R^T in float32 -- the arithmetic
 * gsr_ply_unpack runs on the rows of a file, so gsr_cov_build of the scale / rot it returned gives the cov6 it returned, bit for bit.
 * gsr_cov_build_backward takes grad_cov6 = dLoss/dcov6 in the convention of gsr_raster_backward (an off-diagonal entry stands for both
 * symmetric positions) and returns dLoss/dscaling and dLoss/drotation; the map does not depend on |q|, so rotation . grad_rotation = 0
 * up to rounding and grad_rotation scales with 1 / |q|.
 * scaling[n*3], rotation[n*4], cov6 / grad_cov6[n*6] (xx,xy,xz,yy,yz,zz), grad_scaling[n*3], grad_rotation[n*4]; float32, all host or
 * all device as on_device says (host arrays are staged and copied back; the call returns when the stream has finished).
 *   - n == 0: GSR_OK, no array is touched.  n < 0, or a NULL scaling / rotation / cov6 / grad_cov6 with n > 0: GSR_E_INVALID and a
 *     message that names the argument.
 *   - backward: grad_scaling or grad_rotation may be NULL and is then skipped; both NULL: GSR_E_INVALID.  What is computed for one
 *     output does not depend on whether the other is asked for.
 *   - outputs are overwritten, never accumulated into.
 *   - a row whose six grad_cov6 entries are all zero (the rasteriser gives every culled splat exact zeros) gets exact +0.0 in both
 *     outputs, whatever its scaling and rotation: 0 * exp(100) does not become NaN.
 *   - a row with |q| = 0 or a non-finite input yields what the arithmetic yields (NaN), in that row only -- as the loader does.
 *   - one thread per splat, no atomics: the same inputs give the same bits. */
int32_t gsr_cov_build(const float* scaling, const float* rotation, int64_t n, float* cov6, int32_t on_device, int32_t device, void* stream);
int32_t gsr_cov_build_backward(const float* scaling, const float* rotation, const float* grad_cov6, int64_t n, float* grad_scaling,
                               float* grad_rotation, int32_t on_device, int32_t device, void* stream);

/* 3DGS .ply vertex rows -> the level-0 arrays, on the device (replaces the plyfile -> numpy -> torch.tensor(device=
 * "cuda") chain of GaussianModel.from_ply, src/models/gaussian_model.py:98-139, and the covariance it builds, :34-38 +
 * src/utils/general_utils.py:43-80).  rows_dev: n rows of row_bytes bytes as they are in the file (binary little endian), already in
 * HBM -- the host reads the file in chunks into pinned memory and copies them asynchronously; offsets[15] = byte offsets inside a
 * row of  x y z  f_dc_0..2  opacity  scale_0..2  rot_0..3  f_rest_0  (float32 properties; f_rest_0 .. f_rest_(3K-1) consecutive);
 * K = SH-rest coefficients per channel, 0 <= K <= 1024 (the bound of gsr_ply_pack).  Every offset must satisfy 0 <= offset and
 * offset + 4 <= row_bytes (offset + 12 K <= row_bytes for f_rest_0; that entry is ignored when K = 0), checked in 64-bit arithmetic
 * before anything is launched: GSR_E_INVALID otherwise.  Outputs (device, float32): xyz[n*3], color[n*3] (SH DC), sh[n*3K] coefficient-major
 * (the file is channel-major), opacity[n] (raw), scale[n*3] (log), rot[n*4] (w,x,y,z as stored), cov6[n*6] = R diag(exp(scale))^2 R^T.
 * Enqueued on `stream`; does not synchronise. */
int32_t gsr_ply_unpack(const void* rows_dev, int64_t n, int32_t row_bytes, const int32_t* offsets, int32_t K, float* xyz, float* color,
                       float* sh, float* opacity, float* scale, float* rot, float* cov6, int32_t device, void* stream);

/* The opposite direction: device SoA -> n .ply vertex rows in HBM, in the layout GaussianModel.save_ply writes
 * (src/models/gaussian_model.py:155-185):  x y z  nx ny nz (zero)  f_dc_0..2  f_rest_0..(3K-1) channel-major  opacity  scale_0..2
 * rot_0..3, 17 + 3K little-endian float32 per row.  Inputs (device, float32) as gsr_ply_unpack produces them: xyz[n*3], dc[n*3],
 * sh[n*3K] coefficient-major (NULL when K = 0), opacity[n], scale[n*3], rot[n*4]; rows_dev: n * (17 + 3K) * 4 bytes.  The host
 * copies the rows out through pinned memory chunk by chunk (utils/ply_io.save_gaussian_device).  Enqueued on `stream`; does not
 * synchronise. */
int32_t gsr_ply_pack(const float* xyz, const float* dc, const float* sh, const float* opacity, const float* scale, const float* rot,
                     int64_t n, int32_t K, void* rows_dev, int32_t device, void* stream);

/* ------------------------------------------------------------------------- rigid motion of a splat model */

/* How the SH-rest coefficients of a splat turn with it, on the HOST (no GPU involved).  rotation[9]: a 3x3 rotation, row-major;
 * degree: 0..3; bands[83]: D_1 (3x3), D_2 (5x5), D_3 (7x7), row-major, band after band (bands above `degree`: the identity).
 * Basis = the one 3DGS evaluates -- band 1 is (-C1 y, C1 z, -C1 x), then its five degree-2 and seven degree-3 polynomials --,
 * index = the coefficient index k of _features_rest[n, k, c].  Defining property, for every unit direction d and vector c:
 *     basis_l(R d) . (D_l c) = basis_l(d) . c
 * i.e. the rotated splat seen from the rotated direction shows the original colour.  D_l is orthogonal, D(R1 R2) = D(R1) D(R2), and
 * D_1 = P R P^T with P = [[0,-1,0],[0,0,1],[-1,0,0]] -- NOT R itself.  GSR_E_INVALID for a degree outside 0..3, a NULL pointer, or a
 * matrix with max|R^T R - I| > 1e-3 or det < 0 (a gate against scales and reflections, not a tolerance). */
int32_t gsr_sh_rotation(const double* rotation, int32_t degree, double* bands);

/* A rigid motion applied to a splat model in ONE kernel (GaussianModel.transform_gaussian_model, src/models/gaussian_model.py:198-222):
 *   xyz' = R xyz + t;   cov6' = R cov R^T on the six-entry form (xx,xy,xz,yy,yz,zz);   rot' = normalise(q_R (x) q), quaternions
 *   (w,x,y,z), the motion on the left;   sh: every channel's band vectors multiplied by D_1 / D_2 / D_3 of gsr_sh_rotation when
 *   rotate_sh != 0, copied bit for bit otherwise.
 * transform[16]: row-major 4x4 (float64, narrowed to float32 once; its 3x3 must pass the gate of gsr_sh_rotation); K = SH-rest
 * coefficients per channel: 0, 3, 8 or 15; sh[n*3K] coefficient-major (NULL when K = 0); rot[n*4] may be NULL (rot_out is then
 * ignored).  float32 arithmetic, 64-bit indexing.  All arrays on the host or all on the device as on_device says.  NOT in place:
 * an output that overlaps any other array of the call is GSR_E_INVALID.  Outputs may point into the middle of larger arrays (the
 * merged cloud's rows). */
int32_t gsr_model_transform(const double* transform, int64_t n, int32_t K, int32_t rotate_sh, const float* xyz, const float* cov6,
                            const float* rot, const float* sh, float* xyz_out, float* cov6_out, float* rot_out, float* sh_out,
                            int32_t on_device, int32_t device, void* stream);

/* The same for a SIMILARITY A = c R (a registration with GSR_ICP_POINT_TO_POINT_SCALED; gsr_model_transform keeps refusing it).
 * Gate on the upper 3x3: det A > 0, c = cbrt(det A), 1e-6 <= c <= 1e6, max|A^T A / c^2 - I| <= 1e-3, else GSR_E_INVALID;
 * R = A / c in float64, narrowed to float32 once.  Per splat, in ONE kernel (the rigid kernel's code, instantiated with a factor):
 *   xyz' = c (R xyz) + t;   cov6' = c^2 (R cov R^T);   rot' = normalise(q_R (x) q);   scaling' = scaling + ln c, the LOG-scales
 *   (n, 3) with ln c computed in float64 and narrowed once;   sh by D_l(R) when rotate_sh != 0, copied bit for bit otherwise.
 * Opacity and the DC colour do not change and are not arguments.  scaling / scaling_out may be NULL together, like rot / rot_out.
 * Everything else -- K, placement, NOT in place, outputs into the middle of larger arrays -- as for gsr_model_transform. */
int32_t gsr_model_similarity(const double* transform, int64_t n, int32_t K, int32_t rotate_sh, const float* xyz, const float* cov6,
                             const float* rot, const float* sh, const float* scaling, float* xyz_out, float* cov6_out, float* rot_out,
                             float* sh_out, float* scaling_out, int32_t on_device, int32_t device, void* stream);

/* RANSAC plane search, the data-parallel part: scores ALL candidate planes of one
 * _fit_single_plane call of the reference (src/utils/plane_fitting_util.py:38-69) in one pass over the points.
 * candidates[n_candidates*8] = {n'_0, n'_1, n'_2, d, m_0, m_1, m_2, |n'|}: the plane normal re-normalised as
 * project_point_onto_plane does (:91-96), the offset d, the normal as sampled (used for the alignment test :57-58).
 * counts[c] = points with |distance| < distance_threshold and |<normal_i, m>| > normal_threshold; *best = the first candidate
 * with the strictly largest count (-1 if none has an inlier); best_mask[n] (or NULL) = its inlier mask.
 * xyz / normals[n*3] float32 and best_mask on the host or the device as on_device says; candidates, counts, best: host. */
int32_t gsr_plane_score(const float* xyz, const float* normals, int64_t n, const float* candidates, int32_t n_candidates,
                        float distance_threshold, float normal_threshold, uint32_t* counts, uint8_t* best_mask, int32_t* best,
                        int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------------------ voxel down-sampling */

/* PointCloud::VoxelDownSample (Open3D 0.16.0 PointCloud.cpp), the first step of the reference's voxel multiscale
 * registration (src/gui/workers/registration/qt_multiscale_registrator.py:127-128): voxel_min_bound = min_bound -
 * voxel_size / 2, index = floor((p - voxel_min_bound) / voxel_size) in float64, every voxel averages its points,
 * covariances and colours (float64 sums in input order / count).  Voxels come out in ascending (ix, iy, iz) order
 * (Open3D: unordered_map order).  xyz[n*3], cov6[n*6] or NULL, color[n*3] or NULL, float32.  The result object
 * holds the float64 means on the device until gsr_voxel_free. */
typedef struct gsr_voxel_result gsr_voxel_result;
int32_t gsr_voxel_down_sample(int32_t device, void* stream, const float* xyz, const float* cov6, const float* color,
                              int64_t n, double voxel_size, int32_t on_device, gsr_voxel_result** out,
                              int64_t* n_voxels);
/* xyz[V*3], cov6[V*6] or NULL, color[V*3] or NULL, float64, host or device memory. */
int32_t gsr_voxel_fetch(gsr_voxel_result* r, double* xyz, double* cov6, double* color, int32_t on_device);
int32_t gsr_voxel_free(gsr_voxel_result* r);

/* ------------------------------------------------------------------------------ global registration */

/* The reference's "Global" tab (src/utils/global_registration_util.py: preprocess_point_cloud, do_ransac_registration) through
 * open3d==0.16.0: compute_fpfh_feature, registration_ransac_based_on_feature_matching and
 * registration_ransac_based_on_correspondence.  csrc/features.hip; DESIGN.md section 12.
 *
 * Neighbourhoods are Open3D's KDTreeSearchParamHybrid(radius, max_nn): the max_nn nearest points of the cloud (the query point
 * itself included), ordered by (d2, input index), then cut at the radius, where
 *     d2 = (px - qx)^2 + (py - qy)^2 + (pz - qz)^2     summed left to right in float64 from the float32 coordinates,
 *     a point is kept iff d2 <= radius * radius.
 * (= the points with d2 <= radius^2, the max_nn first of them.)  max_nn in [1, 512]. */
int32_t gsr_hybrid_search(const float* xyz, int64_t n, double radius, int32_t max_nn, int32_t* nbr, int32_t* count, int32_t on_device,
                          int32_t device, void* stream);

/* Open3D 0.16 ComputeFPFHFeature (Feature.cpp) on the hybrid neighbourhoods above, in float64: SPFH of 11 bins per angle
 * (increment 100 / (k - 1), entry 0 of the neighbour list skipped, bins clamped to [0, 10]), then the neighbours' SPFH weighted by
 * 1 / d2 (d2 == 0 skipped), each third normalised to 100, plus the point's own SPFH.  Points with fewer than 2 neighbours get a zero
 * row.  xyz[n*3] float32, normals[n*3] float64, out[n*33] float64 row-major (Open3D's Feature.data is its transpose); host or
 * device memory as on_device says. */
int32_t gsr_fpfh(const float* xyz, const double* normals, int64_t n, double radius, int32_t max_nn, double* out, int32_t on_device,
                 int32_t device, void* stream);

/* Feature matching of registration_ransac_based_on_feature_matching: nn_st[i] = the exact nearest target row of source row i in
 * L2 over the 33 float64 features, d = sum over j = 0..32 in order of (s_j - t_j)^2 (no fused multiply-add), ties to the lowest
 * index (a row whose distances are all NaN or +inf -- NaN features -- gets row 0); with mutual != 0 also nn_ts (target -> source) and the pairs (i, nn_st[i]) with nn_ts[nn_st[i]] == i, in ascending i.
 * corres[ns*2] int32 receives the mutual set when mutual != 0 and it holds at least 3 * ransac_n pairs, else the one-way set
 * (i, nn_st[i]) for every i (Open3D 0.16); *n_corres its length, *used_mutual 1 when it is the mutual set.  nn_st[ns] / nn_ts[nt]
 * may be NULL.  src_feat[ns*33], tgt_feat[nt*33] float64; every array host or device as on_device says, the two counts host. */
int32_t gsr_feature_match(const double* src_feat, int64_t ns, const double* tgt_feat, int64_t nt, int32_t mutual, int32_t ransac_n,
                          int32_t* corres, int64_t* n_corres, int32_t* used_mutual, int32_t* nn_st, int32_t* nn_ts, int32_t on_device,
                          int32_t device, void* stream);

/* Correspondence checkers, applied in the order given to every hypothesis (Open3D CorrespondenceChecker.cpp). */
#define GSR_CHECK_EDGE_LENGTH 0   /* param = similarity threshold: fail if |ps_i - ps_j| < |pt_i - pt_j| * thr or the reverse */
#define GSR_CHECK_DISTANCE    1   /* param = distance threshold: fail if |q - T p| > thr */
#define GSR_CHECK_NORMAL      2   /* param = angle (radians): fail if n_t . (R n_s) < cos(angle); passes when a cloud has no normals */
#define GSR_RANSAC_MAX_N 16       /* largest ransac_n */
typedef struct gsr_ransac_params {
    int32_t kind;              /* GSR_ICP_POINT_TO_POINT (3-pair Umeyama), GSR_ICP_POINT_TO_POINT_SCALED (the same with scaling) or
                                  GSR_ICP_POINT_TO_PLANE (6x6 solve on ransac_n rows) */
    int32_t ransac_n;
    double max_corr;           /* inlier: |T p - q|^2 < max_corr^2 */
    int64_t max_iteration;
    double confidence;
    uint64_t seed;
    int32_t batch;             /* hypotheses per device batch (B); a speed knob only: the result does not depend on it */
    int32_t n_checkers;
    int32_t checker_kind[4];   /* GSR_CHECK_* in the order given */
    double checker_param[4];
} gsr_ransac_params;
typedef struct gsr_ransac_result {
    double T[16];              /* row-major; identity when no hypothesis won */
    double fitness;            /* inliers / |corres| */
    double inlier_rmse;        /* sqrt(sum d2 / inliers); 0 when there are no inliers */
    int64_t best_index;        /* winning hypothesis, -1 if none */
    int64_t n_evaluated;       /* hypotheses k visited (k < exit index) */
    int64_t n_valid;           /* of them: distinct indices and every checker passed */
    int64_t exit_index;        /* final min(max_iteration, early-exit estimate) */
} gsr_ransac_result;
/* Open3D 0.16 RegistrationRANSACBasedOnCorrespondence, deterministic (DESIGN.md 12 lists the deviations):
 *   sampling    hypothesis k draws corres rows  idx_j = draw(seed, k, j, m), j = 0 .. ransac_n - 1, where
 *                 splitmix64(x) = { x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *                                   x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31); }   (mod 2^64)
 *                 draw(seed, k, j, m) = ((splitmix64(seed ^ splitmix64(k * 64 + j)) >> 32) * m) >> 32   (Lemire's reduction)
 *               the draws are sorted ascending; a hypothesis with a repeated row is invalid;
 *   estimate    point-to-point: Umeyama of the ransac_n pairs; point-to-plane: Open3D's 6x6 system on the ransac_n rows;
 *   evaluation  good = #{c : |T p_c - q_c|^2 < max_corr^2}, fitness = good / m, rmse = sqrt(sum d2 / good), in float64;
 *   selection   Open3D's serial rule in index order: better = higher fitness, or equal fitness and lower rmse; after each new best
 *               exit = min(exit, ceil(log(1 - confidence) / log(1 - fitness^ransac_n))) when confidence < 1; stop at k >= exit.
 * With GSR_ICP_POINT_TO_POINT_SCALED every hypothesis is a similarity A = c R: the distance checker and the evaluation use all of
 * it, the normal checker turns the normals by R = A / c (c = cbrt(det A)), and the edge-length checker is applied as written, as
 * Open3D does -- it compares lengths of the two clouds directly, so it is SCALE-SENSITIVE: callers who register clouds of unknown
 * relative scale should leave it out.  Sampling, selection and early exit are the same.  (gsr_fgr_* stay rigid: Open3D's FGR has
 * no scale.)
 * corres[m*2] int32 (source row, target row); xyz float32, normals float64 or NULL; host or device as on_device says.  Degenerate
 * inputs (ransac_n < 3, m < ransac_n, max_corr <= 0) give Open3D's empty result: identity, zeros, best_index -1. */
int32_t gsr_ransac_correspondence(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const double* src_normals,
                                  const double* tgt_normals, const int32_t* corres, int64_t m, const gsr_ransac_params* params,
                                  gsr_ransac_result* out, int32_t on_device, int32_t device, void* stream);

/* Fast Global Registration (Zhou, Park, Koltun 2016) as Open3D 0.16 FastGlobalRegistration.cpp runs it, the second method of the
 * reference's "Global" tab (do_fgr_registration).  csrc/fgr.hip; DESIGN.md section 12.  The matching in front of it is
 * gsr_feature_match with mutual = 1 and ransac_n = 0 (the reciprocal pairs, no fall-back to the one-way set); the evaluation behind
 * it is the ICP context's (gsr_icp_set_target / gsr_icp_set_source / gsr_icp_correspondences).  The fields of gsr_fgr_options are
 * Open3D's FastGlobalRegistrationOption plus seed and batch. */
typedef struct gsr_fgr_options {
    double division_factor;                  /* mu /= division_factor while it is annealed (1.4) */
    int32_t use_absolute_scale;              /* 0: both clouds are divided by scale_global, mu starts at 1; 1: not divided, mu starts at the scale */
    int32_t decrease_mu;                     /* anneal mu every 4th iteration while mu > maximum_correspondence_distance */
    double maximum_correspondence_distance;  /* (0.025) the floor of the annealing; compared with mu as Open3D does: see below */
    int32_t iteration_number;                /* (64) */
    int32_t maximum_tuple_count;             /* (1000) accepted triples kept */
    double tuple_scale;                      /* (0.95) similarity s of the tuple test */
    int32_t tuple_test;                      /* read by callers only: gsr_fgr_tuple_test always tests, gsr_fgr_optimize never does */
    int32_t batch;                           /* trials per device batch; <= 0: 65536.  A speed knob only: the result does not depend on it */
    uint64_t seed;                           /* of draw(seed, k, j, m) */
} gsr_fgr_options;
typedef struct gsr_fgr_result {
    double T[16];              /* row-major, source -> target (what registration_ransac_* returns); identity below 10 pairs */
    int64_t n_corres;          /* pairs the optimiser ran on (its m) */
    int64_t n_reciprocal;      /* the caller's bookkeeping of the stages in front: gsr_fgr_optimize leaves these three untouched */
    int64_t n_trials;
    int64_t n_tuples;
    int32_t iterations;        /* iterations that solved (iteration_number unless a solve failed or m < 10) */
    int32_t host_waits;        /* stream waits of the call: 1 */
    double scale_global;       /* what the coordinates were divided by */
} gsr_fgr_result;
/* The tuple test over m correspondences (source row, target row).  Trial k = 0 .. 100 * m - 1 draws three rows
 *     r_j = draw(seed, k, j, m), j = 0, 1, 2     (the draw of gsr_ransac_correspondence above; unsorted, repeats allowed)
 * and with (i_j, t_j) = corres[r_j] forms, in float64 from the float32 coordinates as given (no normalisation),
 *     li_0 = |P[i_0] - P[i_1]|, li_1 = |P[i_1] - P[i_2]|, li_2 = |P[i_2] - P[i_0]|,  lj_* likewise on Q[t_*],
 *     |d| = sqrt((dx * dx + dy * dy) + dz * dz)  (no fused multiply-add).
 * It is accepted iff  li_e * s < lj_e  and  lj_e < li_e / s  for e = 0, 1, 2  (s = tuple_scale; a repeated row gives a zero edge
 * and fails).  The accepted trials are taken in trial order until maximum_tuple_count of them; each writes its three pairs
 * (i_j, t_j), j = 0, 1, 2, to corres_out[(3 * a + j) * 2 ..].  *n_out = pairs written (3 * accepted); *n_trials = trials the
 * serial loop visits: index of the last accepted trial + 1 when the count is reached, else 100 * m.  This is Open3D's loop with
 * a counter-based generator in place of its random engine; it does not depend on options->batch.
 * corres_out holds 3 * maximum_tuple_count * 2 int32.  xyz float32; the arrays host or device as on_device says, the two counts
 * host.  A row outside [0, ns) x [0, nt) is GSR_E_INVALID (device arrays are checked by the kernel: nothing is read out of bounds). */
int32_t gsr_fgr_tuple_test(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                           const gsr_fgr_options* options, int32_t* corres_out, int64_t* n_out, int64_t* n_trials, int32_t on_device,
                           int32_t device, void* stream);
/* Normalisation, the graduated-non-convexity optimisation and the way back, all in float64:
 *   normalise   each cloud minus its own mean; scale = the largest norm of a centred point of either cloud; use_absolute_scale:
 *               scale_global = 1, mu = scale; else scale_global = scale, mu = 1; points divided by scale_global.
 *   optimise    m < 10: T = identity.  Else p_c / q_c = normalised source / target point of pair c, trans = I, and
 *               iteration_number times:  r = p - q,  l = (mu / (r.r + mu))^2,  rows J0 = [0, -qz, qy, -1, 0, 0],
 *               J1 = [qz, 0, -qx, 0, -1, 0], J2 = [-qy, qx, 0, 0, 0, -1] with residuals rx, ry, rz;  JTJ = sum l J^T J,
 *               JTr = sum l J^T r;  (-JTJ) x = JTr by LDL^T with diagonal pivoting;  delta = [Rz(x2) Ry(x1) Rx(x0) | x3..5];
 *               trans = delta trans;  q_c = delta q_c;  then, if decrease_mu and itr % 4 == 0 and
 *               mu > maximum_correspondence_distance,  mu /= division_factor.  (mu lives in normalised units and is compared with
 *               a distance in the caller's units: Open3D's behaviour, kept.)  A solve with a non-finite solution (zero or
 *               non-finite pivot) ends the loop with the transform reached so far.
 *   way back    R, t of trans:  M = [R | -R mean_t + t scale_global + mean_s]  aligns the target with the source;  T = M^-1.
 * Every sum is taken in a fixed order without atomics: the same inputs give the same bits.  The iterations are enqueued without
 * the host: the call waits for the stream once.  Arguments as for gsr_fgr_tuple_test; ns, nt > 0. */
int32_t gsr_fgr_optimize(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                         const gsr_fgr_options* options, gsr_fgr_result* result, int32_t on_device, int32_t device, void* stream);

/* Compatibility-graph global registration, the project's own definition "after SC2-PCR" (Chen, Sun, Yang, Tao, CVPR 2022): the third
 * global method, deterministic and without sampling.  csrc/sc2.hip; tests/sc2_model.py is this comment in
 * float64 NumPy.  Rigid only.  With p_c = P[corres[c][0]], q_c = Q[corres[c][1]] in float64 from the float32 coordinates:
 *   1 compatibility  a_ij = sqrt((dx * dx + dy * dy) + dz * dz) of p_i - p_j (no fused multiply-add, correctly rounded square root:
 *                    the |d| of gsr_fgr_tuple_test), b_ij the same on q.  C_ij = 1 iff i != j and |a_ij - b_ij| < d_thr.  A NaN
 *                    compares false: a non-finite point is an isolated row.  C is symmetric, C_ii = 0.
 *   2 seeds          deg_i = sum_j C_ij;  n_seeds = min(max_seeds, ceil(seed_ratio * m), m);  the seeds are the first n_seeds
 *                    correspondences in the order (deg descending, index ascending); a seed's place in that order is its RANK.
 *   3 second order   for a seed s:  r_sj = C_sj * sum_k C_sk C_kj  (integers <= m; one product of 0/1 matrices on the i8 MFMA).
 *   4 consensus      K1(s) = s and the first k1 - 1 indices j with C_sj = 1 in the order (r_sj descending, j ascending);
 *                    l_j = #{k in K1(s) : C_jk = 1} for j in K1(s);  K2(s) = s and the first k2 - 1 of K1(s) \ {s} in the order
 *                    (l_j descending, j ascending).  A seed with |K2| < 3 is invalid.
 *   5 hypothesis     T_s = Umeyama without scaling on the members of K2(s) in ascending index: the point-to-point sums about
 *                    ctr = the first member's source point, then the estimator update of the ICP (GSR_ICP_POINT_TO_POINT).  A
 *                    non-finite T_s makes the seed invalid.
 *   6 score          good_s = #{c : |T_s p_c - q_c|^2 < d_thr^2} over all m, rmse_s = sqrt(sum d2 / good_s): the evaluation of
 *                    gsr_ransac_correspondence, sums in a fixed order.  The winner is the best valid seed by (good descending, rmse
 *                    ascending, rank ascending).
 *   7 refinement     at most refine_iters times: Umeyama on all current inliers (sums about the winner's source point, fixed order;
 *                    fewer than 3 inliers or a non-finite result ends it), score the result, keep it iff good rose or good is equal
 *                    and rmse fell, otherwise stop.
 * Every discrete decision up to step 4 is integer arithmetic on C, whose bits step 1 fixes: they do not depend on scheduling.
 * Not covered: similarity hypotheses (the test of step 1 is not scale-invariant), the paper's leading-eigenvector seed score, spatial
 * non-maximum suppression and weighted SVD, point-to-plane estimation, more than GSR_SC2_MAX_CORRES correspondences. */
#define GSR_SC2_MAX_CORRES 32768  /* C is m^2 bytes: 1 GiB here */
#define GSR_SC2_MAX_K 64          /* largest k1 */
typedef struct gsr_sc2_params {
    double d_thr;              /* compatibility and inlier threshold (> 0; otherwise the empty result) */
    double seed_ratio;         /* (0.2) share of the correspondences taken as seeds, in (0, 1] */
    int32_t max_seeds;         /* (4096) cap on the number of seeds, >= 1 */
    int32_t k1;                /* (30) size of the first consensus set */
    int32_t k2;                /* (20) size of the second: 3 <= k2 <= k1 <= GSR_SC2_MAX_K */
    int32_t refine_iters;      /* (20) cap on refinement steps, >= 0 */
} gsr_sc2_params;
typedef struct gsr_sc2_result {
    double T[16];              /* row-major, source -> target; identity when no seed won */
    double fitness;            /* good / m */
    double inlier_rmse;        /* sqrt(sum d2 / good) */
    int64_t best_seed;         /* rank of the winning seed, -1 if none */
    int64_t best_index;        /* its correspondence, -1 if none */
    int64_t n_seeds;
    int64_t n_valid;           /* seeds with |K2| >= 3 and a finite hypothesis */
    int64_t n_edges;           /* sum deg / 2 */
    int32_t refine_steps;      /* refinement steps kept */
    int32_t host_waits;        /* stream waits of the call: one for the winner, one per refinement step tried */
} gsr_sc2_result;
/* corres[m*2] int32 (source row, target row); xyz float32; the arrays host or device as on_device says, params and out host.
 * m < 3 or d_thr <= 0 give the empty result of gsr_ransac_correspondence (identity, zeros, -1); so does a call without a valid
 * seed, which still reports n_seeds, n_edges and host_waits.  GSR_E_INVALID with a message: a row outside [0, ns) x [0, nt) (device
 * arrays are checked by the kernel: nothing is read out of bounds), m > GSR_SC2_MAX_CORRES, a parameter out of range. */
int32_t gsr_sc2_correspondence(const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corres, int64_t m,
                               const gsr_sc2_params* params, gsr_sc2_result* out, int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------- overlap-aware merge */

/* Fuse two splat models that are ALREADY IN ONE FRAME (move one first: gsr_model_transform / gsr_model_similarity): a splat of A
 * and a splat of B that are each other's best match are replaced by their moment-matched union, everything else is kept bit for
 * bit.  csrc/fuse.hip; restated in float64 NumPy in tests/fuse_model.py.  Every quantity is computed in
 * float64 from the float32 inputs and every comparison is written so that NaN fails it.
 *   valid      all of xyz, cov6, opacity finite, det C > 0 (cofactor expansion along the first row) and
 *              w = sigmoid(opacity) sqrt(det C) finite and > 0.  Invalid splats never pair.
 *   candidate  both valid, |ma - mb|^2 <= max_distance^2, |dc_a - dc_b|_2 <= color_delta (inf: no colour gate), J <= kld_max with
 *              J = 1/4 [tr(Cb^-1 Ca) + tr(Ca^-1 Cb) - 6 + d^T (Ca^-1 + Cb^-1) d], d = ma - mb (a negative J, which only rounding
 *              can give, counts as 0).
 *   best       J32 = float32(J); best_b[b] = the candidate a with the smallest (J32, a), best_a[a] the candidate b with the smallest
 *              (J32, b): ties go to the lowest index.  (a, b) is a PAIR iff best_b[b] = a and best_a[a] = b.
 *   fusion     W = wa + wb;  m = (wa ma + wb mb) / W;  C = [wa (Ca + (ma - m)(ma - m)^T) + wb (Cb + (mb - m)(mb - m)^T)] / W;
 *              dc, every sh coefficient and the RAW opacity: the w-weighted mean; narrowed to float32 once.  With scaling / rot the
 *              fused row gets the GSR_DECOMP_EXACT decomposition of its (float32) fused covariance.
 *   output     rows of A not in a pair (ascending a, bit for bit), fused rows (ascending a), rows of B not in a pair (ascending b,
 *              bit for bit): n_out = na + nb - n_pairs.
 * A view: n rows; xyz[n*3], cov6[n*6] (xx,xy,xz,yy,yz,zz), dc[n*3], sh[n*3K] coefficient-major (ignored when K = 0), opacity[n] RAW,
 * scaling[n*3] (log) and rot[n*4] (w,x,y,z): both or neither, and in both input models or in neither; float32.  `out`: the caller's
 * buffers, out->n = their capacity in rows (>= a->n + b->n) on entry and n_out on return; rows behind n_out are not defined.
 * pairs: int32 (min(na, nb), 2) receiving (a, b) in ascending a, or NULL.  All arrays on the host or all on the device as on_device
 * says; the structs themselves on the host.  NOT in place: an output that overlaps another array of the call is GSR_E_INVALID, as
 * are K outside {0, 3, 8, 15}, max_distance <= 0 or not finite, a negative (or NaN) gate, scaling / rot on one side only, a row count
 * >= 2^31 and NULL required arrays.  na = 0 or nb = 0 is valid: the output is the other model.  One wait for the stream in the middle
 * (the counts), one at the end.  Deterministic: the same inputs give the same bits. */
typedef struct gsr_model_view {
    int64_t n;
    float* xyz;
    float* cov6;
    float* dc;
    float* sh;
    float* opacity;
    float* scaling;
    float* rot;
} gsr_model_view;
typedef struct gsr_fuse_params {
    double max_distance;       /* r > 0 */
    double kld_max;            /* >= 0 */
    double color_delta;        /* >= 0; inf disables the colour gate */
} gsr_fuse_params;
typedef struct gsr_fuse_report {
    int64_t n_out, n_pairs, n_a_only, n_b_only, n_invalid_a, n_invalid_b;
    int64_t gated_pairs;       /* the (a, b) that passed all three gates */
    int64_t workspace_bytes;   /* device memory the call allocated beyond the caller's arrays (host callers: the staged copies too) */
    float phase_ms[4];         /* pre-pass + grid, search, pairs + scans, writer: hipEvents on the call's stream */
} gsr_fuse_report;
int32_t gsr_model_fuse(const gsr_model_view* a, const gsr_model_view* b, int32_t K, const gsr_fuse_params* params, gsr_model_view* out,
                       int32_t* pairs, gsr_fuse_report* report, int32_t on_device, int32_t device, void* stream);

/* The pair list of gsr_model_fuse for the same two views and parameters, without an output model: the same pre-pass, grid, search
 * and mutual test (one function behind both entry points), no writer.  Only xyz, cov6, dc and opacity of the views are read.
 * pairs: int32 (min(na, nb), 2) receiving (a, b) in ascending a, or NULL.  report: n_pairs, n_a_only, n_b_only, the invalid counts,
 * gated_pairs and workspace_bytes; n_out = na + nb - n_pairs as the fusion would report it; phase_ms[3] (the writer) is 0.
 * Arrays on the host or on the device as on_device says; refused arguments as in gsr_model_fuse. */
int32_t gsr_model_match(const gsr_model_view* a, const gsr_model_view* b, const gsr_fuse_params* params, int32_t* pairs,
                        gsr_fuse_report* report, int32_t on_device, int32_t device, void* stream);

/* Fuse the overlaps of N models that are ALREADY IN ONE FRAME, in one pass: csrc/fuse_multi.hip; restated in
 * float64 NumPy in tests/fuse_multi_model.py.  Rows get a GLOBAL index g, model-major (the rows of models[0] first, ascending).
 *   valid, gates, J   exactly gsr_model_fuse's; J of a pair is evaluated with the lower global index in the role of `a`.
 *   best[i][m]        for a valid row i and every model m other than its own: the gated candidate j of model m with the smallest
 *                     (J32, j), or none.
 *   mutual edge       {i, j}, i < j, iff best[i][model(j)] = j and best[j][model(i)] = i; its key is (J32, i, j), a strict total order.
 *   groups            by rounds.  Every row starts as a component with the model mask 1 << model.  An edge is LIVE while its ends lie
 *                     in different components with disjoint masks.  In a round every component picks the live edge with the smallest
 *                     key among those that touch it, and an edge picked by BOTH its components merges them (the label becomes the
 *                     lower one -- the lowest member --, the masks are OR-ed).  Rounds repeat until one has no live edge.  A group
 *                     never holds two rows of one model; the partition depends on nothing but the keys.
 *   fusion            a group with members i_1 < ... < i_k, k >= 2: sums in ascending member order in float64, narrowed once:
 *                     W = sum w;  m = (sum w m_i) / W;  C = (sum w (C_i + (m_i - m)(m_i - m)^T)) / W;  dc, every sh coefficient and
 *                     the RAW opacity (sum w v_i) / W.  With scaling / rot: GSR_DECOMP_EXACT of the fused (float32) covariance.
 *   output            the rows in no group of two or more, in global order, bit for bit; then the fused rows, ascending by lowest
 *                     member: n_out = n_total - sum (k - 1).
 * models[n_models], 1 <= n_models <= GSR_FUSE_MAX_MODELS, views as in gsr_model_fuse (scaling / rot: in every model that has rows, or
 * in none).  out->n: the capacity in rows (>= n_total) on entry, n_out on return.  group_of: int32 n_total (or NULL) -- the output row
 * of each input row's group, -1 for a copied row.  n_total and n_total * n_models must be below 2^31.  Everything else (where the
 * arrays live, the overlap rule, the refused arguments) is gsr_model_fuse's; n_models = 1 copies the model.  One stream; the host
 * waits once for the edge count, once per round (the merge count) and once for the group count.  Deterministic. */
#define GSR_FUSE_MAX_MODELS 16
typedef struct gsr_fuse_multi_report {
    int64_t n_out, n_groups, n_grouped_rows;   /* n_out = n_total - n_grouped_rows + n_groups */
    int64_t n_invalid;                         /* over all models */
    int64_t gated_pairs;                       /* the unordered pairs of rows of two models that passed all three gates */
    int64_t mutual_edges;
    int64_t rejected_edges;                    /* mutual edges that died between two components whose masks intersect */
    int64_t rounds;                            /* the rounds that had a live edge */
    int64_t workspace_bytes;                   /* device memory the call allocated beyond the caller's arrays and the staged copies */
    int64_t groups_of_size[GSR_FUSE_MAX_MODELS + 1];      /* [k] = the groups of k members (k >= 2) */
    float phase_ms[6];                         /* pre-pass + grid, search, edge list, rounds, ranks + writer, 0: hipEvents on the stream */
} gsr_fuse_multi_report;
int32_t gsr_fuse_multi(const gsr_model_view* models, int32_t n_models, int32_t K, const gsr_fuse_params* params, gsr_model_view* out,
                             int32_t* group_of, gsr_fuse_multi_report* report, int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------- floater removal: outlier masks and row selection */

/* Which rows of a cloud or splat model survive cleaning: Open3D 0.16's RemoveStatisticalOutlier and RemoveRadiusOutlier, restated
 * (recalled from the published source: parity with Open3D is unpinned), behind a finite test and two splat gates.  csrc/clean.hip;
 * DESIGN.md section 18; restated in float64 NumPy in tests/clean_model.py.  All arithmetic is float64 on the float32 inputs and
 * every comparison is written so that NaN fails it;  d2(i, j) = (xi - xj)^2 + (yi - yj)^2 + (zi - zj)^2 summed left to right.
 * The stages run in this order, each over the survivors of the one before; a dropped row is neither a query nor a candidate.
 *   finite       a row with a non-finite coordinate is dropped (n_nonfinite).  A stated deviation: nanoflann on NaN is undefined.
 *   gates        kept iff raw_opacity >= min_raw_opacity (-inf: off; pass logit(min_opacity)), then iff each of scaling[i, 0..2]
 *                <= max_log_scale (+inf: off; pass ln(max_extent)).  A gate that is on without its array is GSR_E_INVALID.
 *   statistical  on iff nb_neighbors >= 1 (then std_ratio > 0, else GSR_E_INVALID).  A = the rows alive, k' = min(nb_neighbors, |A|);
 *                mean_i = (sum of sqrt(d2) over the k' smallest d2(i, j), j in A INCLUDING j = i, added in ascending order from 0.0)
 *                / k';  valid = |A|;  cloud_mean = sum over mean_i > 0 of mean_i / valid;  std_dev = sqrt(sum over mean_i > 0 of
 *                (mean_i - cloud_mean)^2 / (valid - 1));  threshold = cloud_mean + std_ratio std_dev;  kept iff mean_i > 0 and
 *                mean_i < threshold (valid <= 1: the threshold is NaN and nothing survives).
 *   radius       on iff radius > 0.  count_i = #{j alive : d2(i, j) < radius radius}, self included, STRICT;  kept iff
 *                count_i > nb_points.
 * mask[n] uint8 (1 = kept); mean_dist[n] float64 and count[n] int32, each or NULL: -1 for a row that did not reach its stage.
 * raw_opacity[n], scaling[n*3]: float32 or NULL.  nb_neighbors in [0, 32]; n in [0, 2^31) (n = 0 is valid).  All arrays on the host
 * or all on the device as on_device says; the two structs on the host.  The two moments are reduced in per-block partials whose
 * count depends on n alone and combined in block order, without float atomics: the same input gives the same bits from host or
 * device arrays, run to run.  Host waits: the box read-backs of the grid build, then one at the end (the report). */
typedef struct gsr_clean_params {
    double min_raw_opacity;    /* -inf: gate off */
    double max_log_scale;      /* +inf: gate off */
    int32_t nb_neighbors;      /* 0: no statistical stage */
    int32_t reserved0;
    double std_ratio;
    double radius;             /* <= 0: no radius stage */
    int32_t nb_points;
    int32_t reserved1;
} gsr_clean_params;
typedef struct gsr_clean_report {
    int64_t n, n_nonfinite, n_gate_opacity, n_gate_scale, n_statistical, n_radius, n_kept;      /* rows in, dropped per stage, kept */
    double cloud_mean, std_dev, threshold;      /* of the statistical stage (0 when it is off) */
    int64_t deferred_queries;  /* k-NN queries that left the lane-per-query ring walk for the cooperative kernel */
    int64_t workspace_bytes;   /* device memory the call reserves itself: a function of n and of which arrays are present alone (host
                                  callers: the staged copies too); the grid index of gsr_icp_set_target comes on top */
    float phase_ms[4];         /* pre-pass + grid, k-NN + moments, radius count, mask: hipEvents on the call's stream */
} gsr_clean_report;
int32_t gsr_outlier_mask(const float* xyz, const float* raw_opacity, const float* scaling, int64_t n, const gsr_clean_params* params,
                         uint8_t* mask, double* mean_dist, int32_t* count, gsr_clean_report* report, int32_t on_device, int32_t device,
                         void* stream);
/* The rows of `in` with mask != 0, in ascending order, bit for bit, over every array the view carries (the layout of
 * gsr_model_fuse's views: sh[n*3K] coefficient-major, K in {0, 3, 8, 15}; scaling and rot both or neither; NULL arrays are skipped,
 * in `in` and `out` alike).  out->n = the capacity in rows on entry and n_out on return; index (int32, as many entries as out holds
 * rows, or NULL) receives the kept input rows -- Open3D's second return value; *n_out the count.  More kept rows than `out` holds:
 * GSR_E_INVALID, nothing is written past the capacity.  NOT in place: any overlap between an output and another array of the call
 * is GSR_E_INVALID, as in gsr_model_fuse.  in->n in [0, 2^31).  One wait for the stream in the middle (the count), one at the end. */
int32_t gsr_model_select(const gsr_model_view* in, int32_t K, const uint8_t* mask, gsr_model_view* out, int32_t* index, int64_t* n_out,
                         int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------- multiway registration: pose-graph optimisation (host only) */

/* Pose graph of N scenes (Open3D's PoseGraph + global_optimization; Choi, Zhou, Koltun 2015).  Node i has a rigid pose X_i (row-major
 * 4x4 float64) from its own frame into the global one; edge (source, target, T, information, uncertain) has T from the source's frame
 * into the target's -- what a pairwise registration of (source, target) returns -- so a consistent graph has X_t T = X_s.  Residual of
 * an edge: D = X_t^-1 X_s T^-1, r = [log_SO3(R_D); t_D], chi = r^T information r.  Objective: sum over the certain edges of chi plus,
 * over the uncertain ones, l chi + mu (sqrt(l) - 1)^2 with l = (mu / (mu + chi))^2 in closed form and
 * mu = preference_loop_closure * max_correspondence_distance^2 * mean over the uncertain edges of information[35].  Levenberg-Marquardt
 * on the poses; then every uncertain edge with l < edge_prune_threshold is pruned and the rest is optimised again (mu from the rest).
 * The pose of reference_node is not touched.  csrc/gsr_posegraph.h; no device is involved (like gsr_icp_solve). */
typedef struct gsr_pose_edge {
    int32_t source, target;
    int32_t uncertain;              /* 0: certain ("odometry"), else a loop closure under the line process */
    int32_t reserved;
    double T[16];                   /* source frame -> target frame */
    double information[36];         /* symmetric positive semi-definite, rotation rows / columns first (gsr_icp_information) */
} gsr_pose_edge;
typedef struct gsr_posegraph_option {
    double max_correspondence_distance;        /* Open3D: 0.075 */
    double edge_prune_threshold;               /* 0.25 */
    double preference_loop_closure;            /* 1.0 */
    int32_t reference_node;                    /* 0 */
    int32_t max_iteration, max_iteration_lm;   /* 100, 20 */
    int32_t reserved;
    double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;      /* 1e-6 each */
} gsr_posegraph_option;
typedef struct gsr_posegraph_result {
    int32_t iterations[2];          /* accepted Levenberg-Marquardt steps of the first pass and of the pass after pruning */
    int32_t n_pruned, reserved;
    double E_initial, E_final;      /* the objective (l eliminated) at the input poses / at the returned ones over the remaining edges */
    double mu, mu_first;            /* mu of the last pass (what line_process belongs to) and of the first (what pruned by); 0 without uncertain edges */
} gsr_posegraph_result;
/* poses[n_nodes*16] in and out; line_process[n_edges] (1 for a certain edge; a pruned edge keeps the value it was pruned with),
 * pruned[n_edges] (0 / 1) and result may each be NULL; option NULL = the defaults above.  GSR_E_INVALID with a message: an index out of
 * range, source == target, a node no edge path connects to reference_node, a non-finite pose or transform, an information matrix that is
 * not symmetric positive semi-definite to rounding, a bad option. */
int32_t gsr_posegraph_optimize(int32_t n_nodes, double* poses, int32_t n_edges, const gsr_pose_edge* edges, const gsr_posegraph_option* option,
                               double* line_process, int32_t* pruned, gsr_posegraph_result* result);

/* ------------------------------------------------------------------- splat rasteriser and image metrics (evaluation) */

/* Forward tile rasteriser of a splat model for one pinhole camera: what the reference's Evaluation tab asks of gsplat's
 * rasterization(covars=..., render_mode="RGB", packed=True, radius_clip=3) (src/utils/rasterization_util.py:13-29).  csrc/raster.hip;
 * the semantics are listed in DESIGN.md section 14 and restated in tests/raster_model.py.  gsplat is not available on ROCm: parity
 * with it is unpinned.  The context owns grow-only workspaces (nothing is allocated in steady state); one render at a time per context. */
typedef struct gsr_raster_ctx gsr_raster_ctx;
int32_t gsr_raster_create(gsr_raster_ctx** out, int32_t device, void* stream);
int32_t gsr_raster_destroy(gsr_raster_ctx* ctx);
/* One RGB image.  All arrays are DEVICE pointers in the layout GaussianModel holds: xyz[n*3], cov6[n*6] (xx,xy,xz,yy,yz,zz),
 * raw_opacity[n] (pre-sigmoid), dc[n*3], sh_rest[n*3K] coefficient-major (NULL when sh_degree = 0); K = rest coefficients per channel
 * stored per splat (>= (sh_degree+1)^2 - 1), sh_degree 0..3 = bands evaluated.  viewmat[16] (world -> camera, row-major), background[3]:
 * host.  Fixed: near 0.01, far 1e10, 0.3 px dilation, 16 x 16 tiles, classic (not antialiased) mode; radius_clip: splats whose integer
 * 3-sigma radius is <= it are dropped (the reference passes 3).  image_out[height*width*3] float32 (device), not clamped above.
 * stats_out (device, 3 x int64, or NULL): visible splats, splat-tile intersections, non-empty tiles.  Enqueued on `stream` (NULL: the
 * context's); the call waits for the stream ONCE, in the middle, to read the intersection total that sizes the sort buffers, and
 * returns with the blend enqueued.  If those buffers exceed the device's free memory: GSR_E_HIP with the count in the message.  No
 * float atomics: the same inputs give the same bits. */
int32_t gsr_raster_render(gsr_raster_ctx* ctx, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6,
                          const float* raw_opacity, const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy,
                          float cx, float cy, int32_t width, int32_t height, const float* background, float radius_clip,
                          float* image_out, int64_t* stats_out, void* stream);
/* The same render with the auxiliary outputs of DESIGN.md section 22, each a DEVICE pointer or NULL (all four NULL: GSR_E_INVALID):
 * image_out[height*width*3] -- bit for bit what gsr_raster_render writes (background is required only with it); alpha_out[height*width]
 * = 1 - T with the final transmittance (exactly 0 where no splat counted, otherwise >= 1/255 less the rounding of T, 2^-25); depth_out[height*width] = the expected
 * depth sum(z_i w_i) / max(alpha, 1e-10), z_i the camera-space z, w_i = alpha_i T_i the blending weight (0 where alpha is 0, no
 * background term); contribution_inout[n]: float32 bit patterns, contribution[i] = max(its value before the call, the largest w_i of
 * splat i over the pixels of this image) -- NOT cleared by the call, so several cameras rendered into one buffer leave the maximum
 * over all of them; rows of splats that were culled or never counted are not written.  An integer maximum on the bits of non-negative
 * floats: deterministic.  Validation, messages (under this entry's name), stats_out, stream and timing as for gsr_raster_render. */
int32_t gsr_raster_render_aux(gsr_raster_ctx* ctx, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6,
                              const float* raw_opacity, const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy,
                              float cx, float cy, int32_t width, int32_t height, const float* background, float radius_clip,
                              float* image_out, float* depth_out, float* alpha_out, uint32_t* contribution_inout, int64_t* stats_out,
                              void* stream);
/* ms[3]: preprocess + scan, key emission + sort + tile ranges (the host wait included), blend, of the last render (either entry);
 * waits for it. */
int32_t gsr_raster_get_timing(gsr_raster_ctx* ctx, float* ms);
/* The backward pass of the render (csrc/raster.hip, restated in tests/raster_grad_model.py).  The model and camera
 * arguments are those of gsr_raster_render_aux in the same order.  All pointers but viewmat and background are DEVICE pointers.
 * grad_image[height*width*3] = dL/d image and grad_alpha[height*width] = dL/d coverage (alpha_out): either may be NULL (zeros), not
 * both; background is required only with grad_image.  Outputs, float32 with the shapes of their inputs: grad_xyz[n*3], grad_cov6[n*6],
 * grad_raw_opacity[n], grad_dc[n*3], grad_sh_rest[n*3K]; each may be NULL and is then skipped, at least one must be given; they are
 * OVERWRITTEN, not accumulated.  Validation, messages (under this entry's name), error codes, stats_out and the memory check follow the
 * render entries; the records below take 36 more bytes per splat-tile intersection, counted in that check.  The call is stateless: it
 * runs preprocess, scan, key emission, sort and tile ranges itself on the context's workspaces and relies on no earlier render.
 *
 * Definition: the derivative of the forward pass exactly as tests/raster_model.py states it (coverage: DESIGN.md 22.1), with every
 * discrete decision held at the value the forward took:
 *  - near/far, det <= 0, the radius and bounds culls and the tile box: a culled splat, or a pixel outside a splat's tiles, gets
 *    nothing; a culled splat gets exact +0.0 in every output;
 *  - sigma < 0 and alpha < 1/255: that pixel contributes nothing;
 *  - alpha clamped at 0.999: the splat's colour still gets its gradient at that pixel, nothing flows to sigma or to the opacity;
 *  - the stop at T (1 - alpha) <= 1e-4: the stopping splat and everything behind it get nothing from that pixel; T_end is the
 *    transmittance in front of the stopping splat;
 *  - colour max(v + 0.5, 0): a clamped channel passes nothing to dc, sh_rest or the view direction;
 *  - the frustum clamp of x/z, y/z in the Jacobian: on the clamped branch tx = z lim, whose derivative is 0 in x (or y) and lim in z;
 *  - max(0.01, b^2 - det) affects the radius only: no gradient.
 * Included: the view direction into xyz through the SH basis and the normalisation; the Jacobian's dependence on the point in
 * Sigma_2; the 0.3 I dilation as a constant; cov6's off-diagonal entries receive both symmetric positions; coefficients of sh_rest
 * beyond sh_degree get 0.  Expected depth (depth_out) has NO gradient entry: it is left out.
 * Per pixel, with w_k = alpha_k T_k, C = sum w_k c_k + T_end bg, A = 1 - T_end, G_C = dL/dC, G_A = dL/dA:
 *   dL/dc_k = w_k G_C,   dL/dalpha_k = T_k (c_k . G_C) - [(sum_{m>k} w_m c_m + T_end bg) . G_C - T_end G_A] / (1 - alpha_k)
 * (1 - alpha_k >= 0.001 by the clamp).  The walk goes back to front and recovers T_k by the 3DGS recurrence T <- T / (1 - alpha) from
 * T_end: its rounding differs from the forward's T and is part of the contract (the float32 model repeats it).
 * No float atomics, the same inputs give the same bits: every tile folds the nine per-pixel terms of an intersection (mean2d xy, conic
 * A B C, opacity, r g b) in a fixed tree -- adjacent pairs along a pixel row, then rows in adjacent pairs inside a wave, then the four
 * waves in order -- into one record per intersection, and every splat adds its records in float32 in the row-major order of its tile
 * box before running the projection chain backwards in float32.  One thread walks all tiles of a splat, as in the key emission. */
int32_t gsr_raster_backward(gsr_raster_ctx* ctx, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6,
                            const float* raw_opacity, const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy,
                            float cx, float cy, int32_t width, int32_t height, const float* background, float radius_clip,
                            const float* grad_image, const float* grad_alpha, float* grad_xyz, float* grad_cov6, float* grad_raw_opacity,
                            float* grad_dc, float* grad_sh_rest, int64_t* stats_out, void* stream);
/* ms[4]: preprocess + scan, key emission + sort + tile ranges (the host wait included), blend-backward (the records), splat-backward
 * (the per-splat sums and the chain), of the last gsr_raster_backward on this context; waits for it.  gsr_raster_get_timing is not
 * affected by a backward pass, nor this by a render. */
int32_t gsr_raster_get_backward_timing(gsr_raster_ctx* ctx, float* ms);

/* MSE and SSIM of two (3, height, width) float32 images as the reference's src/utils/evaluation_utils.py defines them: SSIM with the
 * 11 x 11 Gaussian window (sigma 1.5, product of the normalised 1-D window), zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean over all
 * channels and pixels; MSE the mean of the squared float32 differences.  One fused kernel (separable window through LDS, float64)
 * and a fixed-order two-stage float64 reduction.  a, b on the host or the device as on_device says; out[2] = (mse, ssim), host. */
int32_t gsr_image_metrics(const float* a, const float* b, int32_t height, int32_t width, int32_t on_device, double* out, int32_t device,
                          void* stream);

/* ------------------------------------------------------------------- consistent normal orientation */
/* Hoppe's propagation of the normals' signs along the minimum spanning forest of a neighbour graph, on the device.
 * Lists: nbr[n*stride] int32 and count[n] int32 in gsr_hybrid_search's layout (row v holds count[v] entries, clamped to
 * [0, stride]); an entry equal to v or outside [0, n) is skipped (bounds-checked, never dereferenced), duplicates are harmless.
 * A vertex is live when its three normal components are finite.  An undirected edge {i, j} exists when j is in i's list OR i is in
 * j's (the symmetric closure) and both are live.  dot = nix*njx + niy*njy + niz*njz and w = 1 - |dot| in float64, left to right;
 * edges are totally ordered by (w, min(i,j), max(i,j)) (a NaN weight, from overflowing normals, after every number), so the
 * minimum spanning tree of every connected component is unique whatever ties.  A tree edge with dot < 0 joins opposite signs,
 * dot >= 0 equal signs: this fixes every live vertex's flip relative to the lowest-index vertex of its component.
 * Component sign: with reference (host, 3 doubles) every live vertex with finite coordinates votes with
 * t = (cx-px)*nx + (cy-py)*ny + (cz-pz)*nz (float64, left to right, n as oriented so far): t > 0 toward, t < 0 away; away > toward
 * flips the whole component.  On a tie, or with reference == NULL, the component's lowest-index vertex keeps its input sign.
 * Output: every normal is its input or its exact negation (normals[n*3] float64, in place); a non-live vertex is its own component
 * and is never written.  component[n] (int32 or NULL) = the lowest vertex index of the vertex's component.
 * xyz[n*3] float32 may be NULL when reference is NULL.  n in [0, 2^31) and n * stride < 2^30; n == 0: GSR_OK and a zero report.
 * Arrays all on the host or all on the device; the host waits once for the edge count and once per round (at most 32) for a 4-byte
 * counter.  Integer atomics only: the same inputs give the same bits. */
typedef struct gsr_orient_report {
    int64_t n, n_components, n_flipped, n_not_live;   /* components: the non-live singletons included */
    int32_t rounds, reserved;                         /* Boruvka rounds that hooked at least one component */
    int64_t workspace_bytes;                          /* device memory the call reserves itself (host callers: the staged copies too) */
    float phase_ms[4];                                /* lists, CSR and weights, rounds, labels + vote + flip: hipEvents on the stream */
} gsr_orient_report;
int32_t gsr_orient_normals_graph(const float* xyz, double* normals, int64_t n, const int32_t* nbr, int32_t stride, const int32_t* count,
                                 const double* reference, int32_t* component, gsr_orient_report* report, int32_t on_device, int32_t device,
                                 void* stream);
/* The same over the lists of KDTreeSearchParamHybrid(radius, max_nn) (gsr_hybrid_search's, made on the device); xyz is required,
 * radius finite and > 0, max_nn in [1, 512]. */
int32_t gsr_orient_normals(const float* xyz, double* normals, int64_t n, double radius, int32_t max_nn, const double* reference,
                           int32_t* component, gsr_orient_report* report, int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------- colour harmonisation */
/* Exposure / white-balance matching of registered scenes.  csrc/harmonize.hip, csrc/gsr_colorsolve.h; restated in float64 in
 * tests/color_model.py.  Base colour of a splat: x = 0.5 + C0 dc, C0 = 0.28209479177387814, float64 from the float32 dc.  A colour
 * transform of a scene is P = [M | b], row-major 3 x 4 float64, x' = M x + b.
 *
 * gsr_color_sums: the sums of one edge (s, t) over its pairs (i, j) -- row i of s, row j of t -- at the transforms P_s, P_t:
 *   a = [x_i; 1], b = [x_j; 1], u = sigmoid(opacity_s[i]) sigmoid(opacity_t[j]), r = P_s a - P_t b, rho2 = r.r, rho = sqrt(rho2),
 *   h = huber_k / rho if rho > huber_k else 1 (inf: least squares; NaN fails the comparison), w = u h.
 * sums[GSR_COLOR_SUMS_LEN]: [0] n, [1] sum w, [2] sum w rho2, [3..12] sum w a a^T (upper triangle, row by row), [13..28] sum w a b^T
 * (row-major), [29..38] sum w b b^T (upper triangle), [39] 0.  A pair with a non-finite dc or opacity on either side is skipped
 * (*n_skipped); a pair with an index outside its model is never dereferenced, is counted in *n_out_of_range, and the call then
 * returns GSR_E_INVALID.  dc[n*3], opacity[n] float32 and pairs[n_pairs*2] int32 on the host or the device as on_device says; P_s,
 * P_t, sums and the two counts on the host.  One lane per pair, float64 registers, a block fold and a fixed-order final fold: no
 * float atomics, the same bits from run to run and from host or device arrays.  n_pairs = 0: all zeros. */
#define GSR_COLOR_SUMS_LEN 40
int32_t gsr_color_sums(const float* s_dc, const float* s_opacity, int64_t ns, const float* t_dc, const float* t_opacity, int64_t nt,
                       const int32_t* pairs, int64_t n_pairs, const double* P_s, const double* P_t, double huber_k, double* sums,
                       int64_t* n_skipped, int64_t* n_out_of_range, int32_t on_device, int32_t device, void* stream);

/* The transforms of N scenes that minimise
 *   sum_e sum_c [p_s^c' S_aa p_s^c - 2 p_s^c' S_ab p_t^c + p_t^c' S_bb p_t^c] + lambda sum_{i free} |P_i - [I|0]|_F^2,
 * p_i^c = row c of P_i, lambda = prior (sum_e sums[1]) / n_edges: one dense symmetric solve (diagonal-pivoted LDL^T) of size
 * d (number of free nodes), d = 1 (GSR_COLOR_GAIN: P = [g I | 0]), 3 (GSR_COLOR_CHANNEL_GAIN: [diag(g) | 0]) or 12
 * (GSR_COLOR_AFFINE).  Held at their input values: `reference`, and every node that no path of edges with sums[0] >= min_pairs
 * connects to it (held[i] = 1; not an error).  P[n_nodes*12] in and out (held nodes are never written); held: int32 n_nodes or
 * NULL; result may be NULL.  Host code, no device.  GSR_E_INVALID with a message: an index out of range, source == target, a
 * non-finite P or sum, an unknown mode, a negative or non-finite prior, a system that is singular to rounding (raise prior). */
#define GSR_COLOR_GAIN 0
#define GSR_COLOR_CHANNEL_GAIN 1
#define GSR_COLOR_AFFINE 2
typedef struct gsr_color_edge {
    int32_t source, target;
    double sums[GSR_COLOR_SUMS_LEN];
} gsr_color_edge;
typedef struct gsr_color_solve_result {
    double E_initial, E_final;      /* the objective at the input transforms / at the returned ones */
    double pivot_min, pivot_max;    /* of the LDL^T of the solved system (0 when nothing was free) */
    int32_t n_free, n_unknowns;
} gsr_color_solve_result;
int32_t gsr_color_solve(int32_t n_nodes, double* P, int32_t n_edges, const gsr_color_edge* edges, int32_t mode, double prior,
                        int64_t min_pairs, int32_t reference, int32_t* held, gsr_color_solve_result* result);

/* x' = M x + b on a model's colours, exact for every view direction:  dc' = M dc + (M (.5,.5,.5)' + b - (.5,.5,.5)') / C0 and
 * sh'_k = M sh_k for each of the K higher coefficients (sh[n*K*3], the channels innermost).  float64 arithmetic on the float32
 * inputs, each sum left to right, narrowed once; not clamped.  K in {0, 3, 8, 15}; n in [0, 2^31).  dc_out / sh_out may be exactly
 * dc / sh (in place) or disjoint from every input; any other overlap, and a non-finite P12, are GSR_E_INVALID.  NaN rows come out
 * NaN.  Arrays on the host or the device as on_device says; P12 on the host. */
int32_t gsr_model_color_apply(const double* P12, int64_t n, int32_t K, const float* dc, const float* sh, float* dc_out, float* sh_out,
                              int32_t on_device, int32_t device, void* stream);

/* ------------------------------------------------------------------- photometric refinement */
/* The normal equations of one camera of render-based refinement: the hybrid (intensity + depth) term of RGB-D odometry on rendered
 * maps.  csrc/photo.hip; restated in float64 in tests/photo_model.py.  I_t[height*width*3], D_t, A_t[height*width]: colour, expected
 * depth and coverage of the TARGET model as gsr_raster_render_aux writes them; I_s, D_s, A_s: the same of the SOURCE model rendered
 * through viewmat * T, T the current rigid estimate.  viewmat16 (host, row-major, float64) is the camera's own world -> camera matrix
 * [R_c | t_c].  Everything is computed in float64 from the float32 maps, sums of products left to right, no fused multiply-add.
 * A pixel (ix, iy) counts when (float64 comparisons of the widened values, a NaN fails) A_s >= tau, all nine target pixels of its
 * 3 x 3 neighbourhood are inside the image with A_t >= tau, and |D_t - D_s| <= max_depth_diff.  For a counted pixel, with
 * Y = (0.299 r + 0.587 g) + 0.114 b, z = D_s, p = z ((ix + .5 - cx) / fx, (iy + .5 - cy) / fy, 1), p_w = R_c' (p - t_c),
 * M = R_c [-[p_w]x | I] (the increment xi = (omega, v) acts on the left in the world frame: T <- [exp(omega) | v] T), gY and gD the
 * Sobel gradients of the target maps over 8, a = (gY_x fx / z, gY_y fy / z, -(a_0 p_x + a_1 p_y) / z) and d the same of gD with
 * d_2 one less:  J_I = sqrt(1 - lambda) a M,  r_I = sqrt(1 - lambda) (Y_t - Y_s),  J_D = sqrt(lambda) d M,  r_D = sqrt(lambda) (D_t - z).
 * out30 (host): [0..20] the upper triangle of sum(J_I' J_I + J_D' J_D) row by row, [21..26] sum(J_I' r_I + J_D' r_D), [27] sum r_I^2,
 * [28] sum r_D^2, [29] the number of counted pixels.  No counted pixel: thirty zeros, GSR_OK.  D_s > 0 on covered pixels is the
 * renderer's promise and is not checked.  Maps on the host or the device as on_device says.  A lane per pixel, a fixed-order fold
 * per 16 x 16 group and a fixed-order fold of the groups: no atomics, the same inputs give the same bits, from host or device maps.
 * GSR_E_INVALID with a message: a NULL pointer, a non-positive size, lambda outside [0, 1], tau outside (0, 1], max_depth_diff not
 * positive and finite, a non-finite camera or a non-positive focal length -- all before any device call. */
#define GSR_PHOTO_SUMS_LEN 30
int32_t gsr_photo_accumulate(const float* I_s, const float* D_s, const float* A_s, const float* I_t, const float* D_t, const float* A_t,
                             int32_t height, int32_t width, const double* viewmat16, double fx, double fy, double cx, double cy, double lambda,
                             double tau, double max_depth_diff, int32_t on_device, double* out30, int32_t device, void* stream);

/* --------------------------------------------------------------------- non-rigid refinement */
/* A lattice warp that absorbs the smooth drift one matrix leaves between two scenes.  csrc/warp.hip, csrc/gsr_warp.h; restated in
 * float64 in tests/warp_model.py.
 * Lattice: dims3 = (nx, ny, nz) nodes per axis, each in [2, 17], over the box lo3 .. hi3 (hi > lo on every axis); spacing
 * h_a = (hi_a - lo_a) / (n_a - 1); node (ix, iy, iz) has index (ix ny + iy) nz + iz; U[M * 3] (host, float64) are the node
 * displacements.  Cell (cx, cy, cz) has index (cx (ny - 1) + cy) (nz - 1) + cz; its local node k = 4 bx + 2 by + bz.
 * Field, in float64 from the float32 coordinates: s_a = (p_a - lo_a) / h_a, sb_a = min(max(s_a, 0), n_a - 1),
 * c_a = min(floor(sb_a), n_a - 2), f_a = sb_a - c_a; w_k = (X Y) Z with X = f_x or 1 - f_x (b_x = 1 or 0), likewise Y, Z;
 * d(p) = sum_k w_k U_k (k ascending); dw_k/dp_a is the analytic derivative where 0 < s_a < n_a - 1 strictly and 0 elsewhere;
 * F(p) = I + sum_k U_k (grad w_k)'.  A row with a non-finite coordinate is passed through unchanged and takes part in no sum.  A
 * point's cell and weights always come from its UNWARPED position.  No fused multiply-add anywhere.
 *
 * gsr_warp_points: xyz_out = float32(p + d(p)).  gsr_model_warp: that, and cov6_out = F cov F' (float64, rounded once);
 * *n_folded = the finite rows with det F <= 0 (counted, not treated specially).  U == 0 everywhere: the outputs are the inputs'
 * bits.  The outputs may be the inputs themselves.  Arrays on the host or the device as on_device says; lo3, hi3, dims3, U on the host.
 *
 * The context owns the target's point grid with its normals (unit, float64, required) and the source points, which the caller has
 * already moved by the initial matrix.  gsr_warp_accumulate: for every source point with finite coordinates the nearest target point
 * q_j of p + d(p) (float64, not rounded) with d^2 < max_corr^2 strictly, the lowest index on a tie; with n_j its normal,
 * r0 = (p_x - q_x) n_x + (p_y - q_y) n_y + (p_z - q_z) n_z (the UNWARPED p) and g[3 k + a] = w_k n_a.  sums (host,
 * ncells * GSR_WARP_CELL_LEN) holds for every lattice cell: [0..299] the upper triangle of sum g g' row by row, [300..323] sum g r0,
 * [324] sum r0^2, [325] the number of correspondences.  *n_corr = their total; *rmse = sqrt(sum (r0 + g' U)^2 / n_corr), evaluated
 * from the sums (0 without a correspondence).  Order of every sum: the correspondences of a cell in source order, cut into chunks of
 * 1024; the points of a chunk are added in order, then the chunks in order.  No float atomics: the same inputs give the same bits.
 *
 * gsr_warp_solve (host code only, no device is touched): the minimiser of
 *   E(U) = sum_C (r0 + g' U)^2 + lam (n_C / n_T) sum_triples |U_a - 2 U_b + U_c|^2 + 0.01 lam (n_C / n_E) sum_edges |U_a - U_b|^2
 *          + lam0 (n_C / M) sum_nodes |U_a|^2
 * (triples: three consecutive nodes along one axis; edges: axis neighbours; n_T, n_E, M their counts and the nodes'; a term whose
 * count is 0 is dropped) by one banded Cholesky solve.  U: on entry the displacements the sums were taken at (read for E_before
 * only), on exit the minimiser.  n_C = 0 gives U = 0.  GSR_E_INVALID with a message: a dimension outside [2, 17], a non-finite
 * input, a negative weight, a cell whose sums are not those of a symmetric positive semi-definite block to rounding, a system
 * that is not positive definite (lam0 = 0 with empty cells). */
#define GSR_WARP_CELL_LEN 326
typedef struct gsr_warp_ctx gsr_warp_ctx;
typedef struct gsr_warp_report {
    double E_before, E_after;              /* E at the U handed in and at the minimiser */
    double E_data_before, E_data_after;    /* the data term alone */
    int64_t n_corr;
    int32_t n_unknowns, half_band;
    double pivot_min, pivot_max;           /* extreme squared diagonal entries of the Cholesky factor */
} gsr_warp_report;
int32_t gsr_warp_create(gsr_warp_ctx** out, int32_t device, void* stream);
int32_t gsr_warp_destroy(gsr_warp_ctx* ctx);
int32_t gsr_warp_set_target(gsr_warp_ctx* ctx, const float* xyz, const double* normals, int64_t n, double max_corr, int32_t on_device);
int32_t gsr_warp_set_source(gsr_warp_ctx* ctx, const float* xyz, int64_t n, int32_t on_device);
int32_t gsr_warp_accumulate(gsr_warp_ctx* ctx, const double* lo3, const double* hi3, const int32_t* dims3, const double* U, double* sums,
                            int64_t* n_corr, double* rmse);
int32_t gsr_warp_points(const double* lo3, const double* hi3, const int32_t* dims3, const double* U, const float* xyz, int64_t n, float* xyz_out,
                        int32_t on_device, int32_t device, void* stream);
int32_t gsr_model_warp(const double* lo3, const double* hi3, const int32_t* dims3, const double* U, int64_t n, const float* xyz, const float* cov6,
                       float* xyz_out, float* cov6_out, int64_t* n_folded, int32_t on_device, int32_t device, void* stream);
int32_t gsr_warp_solve(const int32_t* dims3, const double* sums, double lam, double lam0, double* U, gsr_warp_report* report);

/* ------------------------------------------------------------- mixture-to-mixture registration */
/* A Gaussian mixture against a Gaussian mixture: every source component interacts with every target component within max_corr,
 * weighted by the overlap of the two Gaussians (Stoyanov et al. 2012; the cross term of Jian and Vemuri's L2 distance).  There is no
 * arg-min and no correspondence.  csrc/d2d.hip, csrc/gsr_d2d.h; restated in float64 in tests/d2d_model.py.
 *
 * Inputs.  Source: centres p_i (float32 xyz), covariances A_i (float32, six entries xx xy xz yy yz zz), weights w_i (float32; NULL:
 * all 1).  Target: q_j, B_j, v_j likewise.  T = [R | t] (float64, 16 values row-major, rigid).  Everything is computed in float64
 * from the widened float32 values; a sum of products runs left to right; no fused multiply-add.
 *
 * Pairs.  p' = R p_i + t.  The pair (i, j) counts when |p' - q_j|^2 < max_corr^2 strictly (d^2 = dx dx + dy dy + dz dz) and the
 * three coordinates, the six covariance entries and the weight are finite on both sides.  ALL such j, not the nearest.
 *
 * Per pair, with s = cov_scale > 0, phi = cov_floor >= 0, S = R A_i R' (G = R A first, then S = G R'), r = p' - q_j:
 *   C_k = (s s) (S_k + B_k), plus phi for k = xx, yy, zz
 *   a_xx = C_yy C_zz - C_yz C_yz   a_xy = C_xz C_yz - C_xy C_zz   a_xz = C_xy C_yz - C_xz C_yy
 *   a_yy = C_xx C_zz - C_xz C_xz   a_yz = C_xy C_xz - C_xx C_yz   a_zz = C_xx C_yy - C_xy C_xy
 *   det = C_xx a_xx + C_xy a_xy + C_xz a_xz;  not (det > 0 and finite): the pair is skipped and counted in n_singular
 *   M_k = a_k (1 / det);  M r row by row;  m = r_x (M r)_x + r_y (M r)_y + r_z (M r)_z;  omega = (w_i v_j) exp(-m / 2)
 *
 * Sums (out32, host, float64), with J = [-[p']x | I3] (rotation columns first, as gsr_icp_information; the increment acts on the
 * left, in the world frame):
 *   [0..20]  upper triangle of H = sum omega J' M J, row by row        [21..26] g = sum omega J' M r
 *   [27]     S = sum omega, the score                                  [28]     sum omega m
 *   [29]     the pairs that count                                      [30]     source rows with at least one such pair
 *   [31]     n_singular
 * Grouping: J depends on the source row only, so a row adds W = sum_j omega M (six), b = sum_j omega M r (three), sum omega and
 * sum omega m over its pairs in the order of the walk, and [0..26] are J' W J and J' b formed once per row (P W, then p' x its rows;
 * P v = p' x v).  The rows are then added in a fixed order that depends on the sizes alone: no float atomics, the same inputs give
 * the same bits, from host arrays or device arrays.  No pair at all gives thirty-two zeros and GSR_OK.
 *
 * gsr_d2d_register, from T = init_T: evaluate; stop without pairs (GSR_D2D_NO_PAIRS); stop when an earlier evaluation exists and
 * |S - S_previous| <= relative_score S (GSR_D2D_CONVERGED); stop after max_iter steps (GSR_D2D_MAX_ITERATION); else solve
 * H xi = -g by LDL' with diagonal pivoting (a non-finite xi: GSR_D2D_DEGENERATE, no step), form
 *   dT = [Rz(xi_2) Ry(xi_1) Rx(xi_0) | (xi_3, xi_4, xi_5)]
 * -- the matrix the ICP step forms from its six-vector -- and T <- dT T.  M and omega are frozen within a step (IRLS, as
 * Generalized ICP freezes its M).  The report is taken at the final T: score = S, fitness = [30] / n_source,
 * mahalanobis_rmse = sqrt([28] / [27]) (a Mahalanobis quantity, not a distance), iterations = the steps taken.
 *
 * The context owns the target's point grid, the target's covariances and weights in cell order, and a copy of the source in the
 * order of the target's cells; the arrays are on the host or the device as on_device says and are not needed after the call.  A new
 * target keeps the source.  n = 0 is allowed on either side (no pairs).  There is no communicator entry: one context, one device.
 * GSR_E_INVALID with a message, before any device call: a NULL pointer, a negative size, max_corr or cov_scale not positive and
 * finite, cov_floor or relative_score negative or not finite, a negative max_iter, a non-finite T. */
#define GSR_D2D_SUMS_LEN 32
#define GSR_D2D_CONVERGED 0
#define GSR_D2D_MAX_ITERATION 1
#define GSR_D2D_NO_PAIRS 2
#define GSR_D2D_DEGENERATE 3
typedef struct gsr_d2d_ctx gsr_d2d_ctx;
typedef struct gsr_d2d_report {
    double score, fitness, mahalanobis_rmse;
    int64_t n_pairs, n_singular;
    int32_t iterations, status;
} gsr_d2d_report;
int32_t gsr_d2d_create(gsr_d2d_ctx** out, int32_t device, void* stream);
int32_t gsr_d2d_destroy(gsr_d2d_ctx* ctx);
int32_t gsr_d2d_set_target(gsr_d2d_ctx* ctx, const float* xyz, const float* cov6, const float* weight, int64_t n, double max_corr, int32_t on_device);
int32_t gsr_d2d_set_source(gsr_d2d_ctx* ctx, const float* xyz, const float* cov6, const float* weight, int64_t n, int32_t on_device);
int32_t gsr_d2d_accumulate(gsr_d2d_ctx* ctx, const double* T, double cov_scale, double cov_floor, double* out32);
int32_t gsr_d2d_register(gsr_d2d_ctx* ctx, const double* init_T, double cov_scale, double cov_floor, double relative_score, int32_t max_iter,
                         double* out_T, gsr_d2d_report* report);

/* ------------------------------------------------------- photometric loss of the fine-tuner */
/* loss = (1 - lambda) L1 + lambda (1 - SSIM) of an image against a target, and its gradient with respect to the image, in one fused
 * kernel.  csrc/imgloss.hip; restated in tests/ssim_loss_model.py.  The SSIM is the one gsr_image_metrics defines (11 x 11 Gaussian
 * window, sigma 1.5, the outer product of the normalised 1-D window -- both entries take it from one host function --, zero padding,
 * C1 = 0.01^2, C2 = 0.03^2, mean over all 3 H W terms), here on the INTERLEAVED (H, W, 3) layout the rasteriser writes.
 *
 * For an image a and a target b, both (height, width, 3) float32, N = 3 height width, one channel at a time, G* the zero-padded
 * 11 x 11 filter (horizontal pass first, taps in ascending order):
 *   mu1 = G*a   mu2 = G*b   m_aa = G*(a a)   m_bb = G*(b b)   m_ab = G*(a b)
 *   s1 = m_aa - mu1^2   s2 = m_bb - mu2^2   s12 = m_ab - mu1 mu2
 *   A1 = 2 mu1 mu2 + C1   A2 = 2 s12 + C2   B1 = mu1^2 + mu2^2 + C1   B2 = s1 + s2 + C2
 *   S = A1 A2 / (B1 B2)
 *   l1 = sum |a - b| / N     ssim = sum S / N     loss = (1 - lambda) l1 + lambda (1 - ssim)
 * Gradient with respect to a (the target gets none).  Three maps, ZERO outside the image (a padded pixel has no SSIM term):
 *   D1 = 2 mu2 A2 / (B1 B2) - 2 mu2 A1 / (B1 B2) - 2 mu1 S / B1 + 2 mu1 S / B2      D2 = -S / B2      D3 = 2 A1 / (B1 B2)
 *   dloss/da = (1 - lambda) sign(a - b) / N - (lambda / N) (G*D1 + 2 a (G*D2) + b (G*D3)),   sign(0) = 0
 * (the window is symmetric, so the zero-padded filter is its own adjoint).
 *
 * Arithmetic: float64 from the widened float32 pixels up to ONE rounding to float32 at the store of the gradient; no fused
 * multiply-add; the sums l1 and ssim are folded in the fixed order of csrc/gsr_fold.h (every thread its own pixel over the channels
 * in ascending order, the xor tree per wave, the four waves in order, k_fold_partials<256> over the tiles in row-major order): no
 * atomics, the same inputs give the same bits.  Non-finite pixels are not treated specially.
 *
 * gsr_loss_create / gsr_loss_destroy: an owning context with a grow-only buffer of two float64 per 16 x 16 tile.
 * gsr_loss_l1_dssim: image, target, loss_out and grad_image are DEVICE pointers on the context's device.  loss_out: double[3] =
 * (loss, l1, ssim).  grad_image: (height, width, 3) float32, every entry OVERWRITTEN; NULL: the adjoint half is skipped and
 * loss_out has the same bits.  The call is enqueued on `stream`, waits for nothing and allocates nothing once the context has grown
 * to the image size (growing it frees the old buffer, which waits for the device).  GSR_E_INVALID with a message, before any device
 * call: a NULL context, image, target or loss_out, a non-positive size, lambda outside [0, 1] (a NaN included), more than 65535 rows
 * of tiles.  No device visible: GSR_E_NO_DEVICE. */
typedef struct gsr_loss_ctx gsr_loss_ctx;
int32_t gsr_loss_create(int32_t device, gsr_loss_ctx** out);
int32_t gsr_loss_destroy(gsr_loss_ctx* ctx);
int32_t gsr_loss_l1_dssim(gsr_loss_ctx* ctx, const float* image, const float* target, int32_t height, int32_t width, double lambda,
                          double* loss_out, float* grad_image, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_HIP_H */
