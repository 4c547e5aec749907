// fuse.hip -- overlap-aware merge of two registered splat models (gsr_model_fuse, include/gsr_hip.h).
//
// A splat of model A and a splat of model B that are each other's best match under a distance gate, a colour gate and a gate on the
// symmetrised KL divergence J are replaced by their moment-matched union (the operation of HEM's M-step, across two models);
// everything else is copied bit for bit.  The definition is restated in float64 NumPy in tests/fuse_model.py.
//
//   k_fuse_prep        per splat of both models: validity, w = sigmoid(opacity) sqrt(det), the float64 inverse covariance
//   k_fuse_moments /   the box of the grid over A without the host: moments of the valid centres, then of those within 3 sigma of the
//   k_fuse_box         first pass (far outliers leave), box = mean +- 4 sigma cut to the extremes; edge >= max_distance, enlarged
//                      until the table has at most `cap` = max(na, 1024) cells.  Coordinates outside the box clamp into boundary
//                      cells: clamping is monotone, so two centres within one edge of each other stay in adjacent cells.
//   k_fuse_keys, sort, k_fuse_cell_starts, k_fuse_gather_a    A in cell order: a cell is a contiguous span of the search arrays
//   k_fuse_search      a thread per splat of B in the order of A's cell key: 9 spans (3 x-adjacent cells each), gates cheapest first,
//                      its own best (J32, a) in registers, one no-return 64-bit atomicMin of (J32 bits << 32 | b) into best_a[a] per
//                      GATED pair.  J >= 0, so the float bits order like the value; min is exact and order-free: deterministic.
//   k_fuse_pair        mutual test (best_a is complete here: the kernel boundary is the only synchronisation), flags, the pair list
//   scan_exclusive x2, k_fuse_rows    a lane per output FLOAT: unpaired rows are copied as 32-bit words, fused rows are computed in
//                      float64 and narrowed once.  Output: A-only rows, fused rows (ascending a), B-only rows.
// The host reads the counts back once; scaling / rot of the fused rows are then gsr_decompose_cov (GSR_DECOMP_EXACT) of the fused
// covariances, which lie in one contiguous block of the output.
#include "gsr_common.h"
#include "gsr_oneshot.h"
#include "gsr_fuse_args.h"
#include "gsr_fuse_dev.h"
#include "gsr_prims.h"

#include <float.h>
#include <math.h>
#include <string.h>

namespace gsr {

// A's search arrays in cell order; an invalid splat gets NaN centres, which fail the distance gate
__global__ __launch_bounds__(256) void k_fuse_gather_a(int64_t n, const unsigned* __restrict__ order, const float* __restrict__ xyz, const float* __restrict__ dc,
                                                       const float* __restrict__ cov6, const double* __restrict__ w, const double* __restrict__ inv,
                                                       float* __restrict__ sxyz, float* __restrict__ sdc, float* __restrict__ scov, double* __restrict__ sinv) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = order[p];
        const bool valid = w[a] > 0.0;
        const float nan = __builtin_nanf("");
        for (int k = 0; k < 3; ++k) { sxyz[3 * p + k] = valid ? xyz[3 * a + k] : nan; sdc[3 * p + k] = dc[3 * a + k]; }
        for (int k = 0; k < 6; ++k) { scov[6 * p + k] = cov6[6 * a + k]; sinv[6 * p + k] = inv[6 * a + k]; }
    }
}

__global__ __launch_bounds__(256) void k_fuse_search(int64_t nb, const unsigned* __restrict__ orderB, const float* __restrict__ xyzB, const float* __restrict__ dcB,
                                                     const float* __restrict__ covB, const double* __restrict__ wB, const double* __restrict__ invB,
                                                     const FuseGrid* __restrict__ G, const int* __restrict__ cellStart, const float* __restrict__ sxyz,
                                                     const float* __restrict__ sdc, const float* __restrict__ scov, const double* __restrict__ sinv,
                                                     const unsigned* __restrict__ orderA, double r2, double kld_max, double cd2,
                                                     unsigned long long* __restrict__ best_a, int* __restrict__ best_b, unsigned long long* __restrict__ n_gated) {
    const FuseGrid g = *G;
    unsigned gated = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nb; t += (int64_t)gridDim.x * blockDim.x) {
        const unsigned b = orderB[t];
        int best = -1;
        if (wB[b] > 0.0) {
            const double bx = xyzB[3 * (int64_t)b], by = xyzB[3 * (int64_t)b + 1], bz = xyzB[3 * (int64_t)b + 2];
            const double e0 = dcB[3 * (int64_t)b], e1 = dcB[3 * (int64_t)b + 1], e2 = dcB[3 * (int64_t)b + 2];
            double Bc[6], Bi[6];
            for (int k = 0; k < 6; ++k) { Bc[k] = covB[6 * (int64_t)b + k]; Bi[k] = invB[6 * (int64_t)b + k]; }
            const int cx = fuse_cell(bx, g.ox, g.inv_c, g.gx), cy = fuse_cell(by, g.oy, g.inv_c, g.gy), cz = fuse_cell(bz, g.oz, g.inv_c, g.gz);
            const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.gx - 1 ? cx + 1 : g.gx - 1;
            const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < g.gy - 1 ? cy + 1 : g.gy - 1;
            const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < g.gz - 1 ? cz + 1 : g.gz - 1;
            unsigned long long mine = ~0ull;                    // (J32 bits << 32) | a
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.gy + y) * g.gx;
                    const int p1 = cellStart[row + x1 + 1];
                    for (int p = cellStart[row + x0]; p < p1; ++p) {
                        const double dx = (double)sxyz[3 * (int64_t)p] - bx, dy = (double)sxyz[3 * (int64_t)p + 1] - by, dz = (double)sxyz[3 * (int64_t)p + 2] - bz;
                        if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
                        const double f0 = (double)sdc[3 * (int64_t)p] - e0, f1 = (double)sdc[3 * (int64_t)p + 1] - e1, f2 = (double)sdc[3 * (int64_t)p + 2] - e2;
                        if (!((f0 * f0 + f1 * f1) + f2 * f2 <= cd2)) continue;
                        double Ac[6], Ai[6];
                        for (int k = 0; k < 6; ++k) { Ac[k] = scov[6 * (int64_t)p + k]; Ai[k] = sinv[6 * (int64_t)p + k]; }
                        double J = 0.25 * (((sym_trace(Bi, Ac) + sym_trace(Ai, Bc)) - 6.0) + (sym_quad(Ai, dx, dy, dz) + sym_quad(Bi, dx, dy, dz)));
                        if (J < 0.0) J = 0.0;                   // rounding only: J >= 0 in exact arithmetic
                        if (!(J <= kld_max)) continue;
                        const unsigned long long jb = (unsigned long long)__float_as_uint((float)J) << 32;
                        const unsigned a = orderA[p];
                        const unsigned long long k = jb | a;
                        if (k < mine) mine = k;
                        atomicMin(&best_a[a], jb | b);
                        ++gated;
                    }
                }
            if (mine != ~0ull) best = (int)(unsigned)(mine & 0xffffffffull);
        }
        best_b[b] = best;
    }
    for (int o = 32; o > 0; o >>= 1) gated += __shfl_xor(gated, o);
    if ((threadIdx.x & 63) == 0 && gated) atomicAdd(n_gated, (unsigned long long)gated);
}

// the mutual test: a and b pair iff each is the other's best
__global__ __launch_bounds__(256) void k_fuse_pair(int64_t na, const unsigned long long* __restrict__ best_a, const int* __restrict__ best_b,
                                                   int* __restrict__ flagA, int* __restrict__ flagB, int* __restrict__ mate) {
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < na; a += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = best_a[a];
        int b = -1;
        if (k != ~0ull) {
            const unsigned c = (unsigned)(k & 0xffffffffull);
            if (best_b[c] == (int)a) b = (int)c;
        }
        mate[a] = b;
        if (b >= 0) { flagA[a] = 1; flagB[b] = 1; }
    }
}

__global__ __launch_bounds__(256) void k_fuse_pairs_out(int64_t na, const int* __restrict__ mate, const int* __restrict__ scanA, int32_t* __restrict__ pairs) {
    for (int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; a < na; a += (int64_t)gridDim.x * blockDim.x)
        if (mate[a] >= 0) { pairs[2 * (int64_t)scanA[a]] = (int32_t)a; pairs[2 * (int64_t)scanA[a] + 1] = mate[a]; }
}

// One array of the output, a lane per float of the two inputs laid end to end (consecutive lanes on consecutive addresses of a row).
//   an unpaired row        its W words, copied as integers
//   a paired row of A      MODE 1: the w-weighted mean of the two rows' floats (xyz, dc, sh, opacity), MODE 2 (W = 6): the moment-
//                          matched covariance [wa (Ca + da da^T) + wb (Cb + db db^T)] / (wa + wb), d = the centre minus the fused
//                          centre -- a sum of PSD terms -- both in float64, narrowed once; MODE 0: left for gsr_decompose_cov
//   a paired row of B      nothing
#define FUSE_COPY 0
#define FUSE_MEAN 1
#define FUSE_COV 2
__global__ __launch_bounds__(256) void k_fuse_rows(int64_t na, int64_t nb, int W, int mode, const float* __restrict__ A, const float* __restrict__ B,
                                                   float* __restrict__ O, const int* __restrict__ mate, const int* __restrict__ scanA,
                                                   const int* __restrict__ flagB, const int* __restrict__ scanB, const double* __restrict__ wA,
                                                   const double* __restrict__ wB, const float* __restrict__ xyzA, const float* __restrict__ xyzB) {
    const int64_t total = (na + nb) * W;
    const int64_t a_only = na - scanA[na];                       // scanA[na] = the number of pairs
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / W;
        const int j = (int)(t - i * W);
        if (i >= na) {
            const int64_t b = i - na;
            if (!flagB[b]) reinterpret_cast<uint32_t*>(O)[(na + b - scanB[b]) * W + j] = reinterpret_cast<const uint32_t*>(B)[b * W + j];
            continue;
        }
        const int64_t b = mate[i];
        if (b < 0) { reinterpret_cast<uint32_t*>(O)[(i - scanA[i]) * W + j] = reinterpret_cast<const uint32_t*>(A)[t]; continue; }
        if (mode == FUSE_COPY) continue;
        const double wa = wA[i], wb = wB[b], ws = wa + wb;
        double v;
        if (mode == FUSE_MEAN) v = (wa * (double)A[t] + wb * (double)B[b * W + j]) / ws;
        else {
            const int r = j < 3 ? 0 : j < 5 ? 1 : 2, c = j < 3 ? j : j < 5 ? j - 2 : 2;      // (xx, xy, xz, yy, yz, zz)
            const double ar = xyzA[3 * i + r], ac = xyzA[3 * i + c], br = xyzB[3 * b + r], bc = xyzB[3 * b + c];
            const double mr = (wa * ar + wb * br) / ws, mc = (wa * ac + wb * bc) / ws;
            v = (wa * ((double)A[t] + (ar - mr) * (ac - mc)) + wb * ((double)B[b * W + j] + (br - mr) * (bc - mc))) / ws;
        }
        O[(a_only + scanA[i]) * W + j] = (float)v;
    }
}


// Everything gsr_model_fuse does before its writer, and all of gsr_model_match: staging, pre-pass, grid, search, mutual test, scans,
// pair list (run), then the one read-back (counts).  What the writer and the report read stays here: the caller declares its
// FuseFront BEFORE its OneShot.
struct FuseFront {
    DevBuf tmp_sort_a, tmp_sort_b, tmp_scan_a, tmp_scan_b;
    Event ev[5];                                                // run() records 0..2; the caller records 3 and, behind a writer, 4
    size_t workspace = 0;                                       // device bytes asked for beyond the caller's arrays (rocPRIM's temporaries are added at the end)
    const float *da[GSR_MODEL_NARR], *db[GSR_MODEL_NARR];       // the used arrays of the two models on the device
    int32_t* dpairs = nullptr;
    double *wA = nullptr, *wB = nullptr;
    int *mate = nullptr, *scanA = nullptr, *flagB = nullptr, *scanB = nullptr;
    unsigned long long* counters = nullptr;                     // invalid A, invalid B, gated pairs
    unsigned long long hc[3] = {0, 0, 0};                       // the counters and the pair count on the host: read back asynchronously, so they
    int hp = 0;                                                 // live here, beyond the OneShot's last wait, not in a frame that may be left early

    int32_t run(OneShot& os, const gsr_model_view* a, const gsr_model_view* b, const size_t width[GSR_MODEL_NARR], const bool used[GSR_MODEL_NARR],
                const gsr_fuse_params* params, int32_t* pairs) {
        hipStream_t st = os.st;
        auto ws = [&](size_t bytes, auto** p) { workspace += bytes; return os.scratch(bytes, p); };
        const int64_t na = a->n, nb = b->n;
        GSR_TRY(model_in(os, a, width, used, da));
        GSR_TRY(model_in(os, b, width, used, db));
        const size_t npair_cap = (size_t)(na < nb ? na : nb);
        if (pairs && npair_cap) { if (os.on_device) dpairs = pairs; else GSR_TRY(os.scratch(npair_cap * 8, &dpairs)); }
        double *invA, *invB, *sinv;
        float *sxyz, *sdc, *scov;
        unsigned *keysB, *idxB, *skeysB, *orderB;
        int *best_b, *flagA;
        unsigned long long* best_a;
        FuseCells c;                                            // the grid over A
        const size_t ua = (size_t)na, ub = (size_t)nb;
        GSR_TRY(ws(ua * 8 + 8, &wA)); GSR_TRY(ws(ub * 8 + 8, &wB));
        GSR_TRY(ws(ua * 48 + 8, &invA)); GSR_TRY(ws(ub * 48 + 8, &invB));
        GSR_TRY(ws(ua * 48 + 8, &sinv)); GSR_TRY(ws(ua * 12 + 8, &sxyz)); GSR_TRY(ws(ua * 12 + 8, &sdc)); GSR_TRY(ws(ua * 24 + 8, &scov));
        GSR_TRY(ws(ub * 4 + 8, &keysB)); GSR_TRY(ws(ub * 4 + 8, &idxB)); GSR_TRY(ws(ub * 4 + 8, &skeysB)); GSR_TRY(ws(ub * 4 + 8, &orderB));
        GSR_TRY(ws(ua * 8 + 8, &best_a)); GSR_TRY(ws(ub * 4 + 8, &best_b)); GSR_TRY(ws(ua * 4 + 8, &mate));
        GSR_TRY(ws((ua + 1) * 4, &flagA)); GSR_TRY(ws((ub + 1) * 4, &flagB)); GSR_TRY(ws((ua + 1) * 4, &scanA)); GSR_TRY(ws((ub + 1) * 4, &scanB));
        GSR_TRY(ws(3 * 8, &counters));
        GSR_TRY(c.reserve(os, workspace, na));
        GSR_HIP(hipMemsetAsync(counters, 0, 3 * 8, st));
        GSR_HIP(hipMemsetAsync(flagA, 0, (ua + 1) * 4, st));
        GSR_HIP(hipMemsetAsync(flagB, 0, (ub + 1) * 4, st));
        GSR_HIP(hipMemsetAsync(best_a, 0xff, ua * 8 + 8, st));

        // ---- pre-pass and grid; B gets keys of A's grid and the order they give
        GSR_HIP(hipEventRecord(ev[0], st));
        GSR_TRY(c.launch(st, tmp_sort_a, da[0], da[1], da[4], wA, invA, counters, params->max_distance));
        hipLaunchKernelGGL(k_fuse_prep, dim3(stride_grid(nb)), dim3(256), 0, st, nb, db[0], db[1], db[4], wB, invB, counters + 1);
        hipLaunchKernelGGL(k_fuse_keys, dim3(stride_grid(nb)), dim3(256), 0, st, nb, db[0], (const FuseGrid*)c.grid, keysB, idxB);
        if (nb > 0) GSR_TRY(sort_pairs_by_key<rocprim::default_config>(tmp_sort_b, st, (const unsigned*)keysB, skeysB, (const unsigned*)idxB, orderB, ub, 0u, c.bits));
        hipLaunchKernelGGL(k_fuse_gather_a, dim3(stride_grid(na)), dim3(256), 0, st, na, (const unsigned*)c.order, da[0], da[2], da[1], wA, invA, sxyz, sdc, scov, sinv);
        // ---- search
        GSR_HIP(hipEventRecord(ev[1], st));
        const double r2 = params->max_distance * params->max_distance, cd2 = params->color_delta * params->color_delta;
        hipLaunchKernelGGL(k_fuse_search, dim3(stride_grid(nb)), dim3(256), 0, st, nb, orderB, db[0], db[2], db[1], wB, invB, (const FuseGrid*)c.grid,
                           (const int*)c.cellStart, sxyz, sdc, scov, sinv, (const unsigned*)c.order, r2, params->kld_max, cd2, best_a, best_b, counters + 2);
        // ---- pairs and scans
        GSR_HIP(hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_fuse_pair, dim3(stride_grid(na)), dim3(256), 0, st, na, best_a, best_b, flagA, flagB, mate);
        GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan_a, st, (const int*)flagA, scanA, ua + 1));
        GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan_b, st, (const int*)flagB, scanB, ub + 1));
        if (dpairs) hipLaunchKernelGGL(k_fuse_pairs_out, dim3(stride_grid(na)), dim3(256), 0, st, na, mate, scanA, dpairs);
        return GSR_OK;
    }

    // the one read-back: the counts into the report with the first `phases` phase times, the pair list to a host caller
    int32_t counts(OneShot& os, int64_t na, int64_t nb, int phases, gsr_fuse_report* r, int32_t* pairs) {
        GSR_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, os.st));
        GSR_HIP(hipMemcpyAsync(&hp, scanA + na, 4, hipMemcpyDeviceToHost, os.st));
        GSR_TRY(os.wait());
        const int64_t np = hp;
        r->n_pairs = np; r->n_out = na + nb - np; r->n_a_only = na - np; r->n_b_only = nb - np;
        r->n_invalid_a = (int64_t)hc[0]; r->n_invalid_b = (int64_t)hc[1];
        for (int k = 0; k < phases; ++k) (void)hipEventElapsedTime(&r->phase_ms[k], ev[k], ev[k + 1]);
        r->gated_pairs = (int64_t)hc[2];
        r->workspace_bytes = (int64_t)(workspace + tmp_sort_a.cap + tmp_sort_b.cap + tmp_scan_a.cap + tmp_scan_b.cap);
        if (!os.on_device && dpairs && np > 0) GSR_HIP(hipMemcpyAsync(pairs, dpairs, (size_t)np * 8, hipMemcpyDeviceToHost, os.st));
        return GSR_OK;
    }
};

}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_model_fuse(const gsr_model_view* a, const gsr_model_view* b, int32_t K, const gsr_fuse_params* params, gsr_model_view* out,
                                  int32_t* pairs, gsr_fuse_report* report, int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_model_fuse";
    size_t width[GSR_MODEL_NARR];
    bool used[GSR_MODEL_NARR], with_sr = false;
    char why[256];
    if (const char* refused = fuse_check_args(a, b, K, params, out, pairs, report, width, used, &with_sr, why, sizeof why))
        return fail(GSR_E_INVALID, "gsr_model_fuse: %s", refused);
    const int64_t na = a->n, nb = b->n, cap_rows = na + nb;
    const int modes[GSR_MODEL_NARR] = {FUSE_MEAN, FUSE_COV, FUSE_MEAN, FUSE_MEAN, FUSE_MEAN, FUSE_COPY, FUSE_COPY};
    GSR_TRY(open_device(device, who));
    memset(report, 0, sizeof(*report));
    if (cap_rows == 0) { out->n = 0; return GSR_OK; }

    FuseFront f;                                                // (rocPRIM's temporaries: declared before the OneShot, freed after its wait)
    for (Event& e : f.ev) GSR_HIP(e.create());
    OneShot os((hipStream_t)stream, on_device != 0, who);
    hipStream_t st = os.st;
    float* dout[GSR_MODEL_NARR];
    GSR_TRY(model_out(os, out, cap_rows, width, used, dout));
    GSR_TRY(f.run(os, a, b, width, used, params, pairs));
    // ---- writer
    GSR_HIP(hipEventRecord(f.ev[3], st));
    for (int k = 0; k < GSR_MODEL_NARR; ++k)
        if (used[k])
            hipLaunchKernelGGL(k_fuse_rows, dim3(stride_grid(cap_rows * (int64_t)width[k])), dim3(256), 0, st, na, nb, (int)width[k], modes[k], f.da[k], f.db[k], dout[k],
                               (const int*)f.mate, (const int*)f.scanA, (const int*)f.flagB, (const int*)f.scanB, (const double*)f.wA, (const double*)f.wB, f.da[0],
                               f.db[0]);
    GSR_HIP(hipEventRecord(f.ev[4], st));
    GSR_TRY(f.counts(os, na, nb, 4, report, pairs));
    const int64_t np = report->n_pairs, n_out = report->n_out;
    if (with_sr && np > 0) {
        const int64_t off = na - np;
        GSR_TRY(gsr_decompose_cov(dout[1] + 6 * off, np, GSR_DECOMP_EXACT, dout[5] + 3 * off, dout[6] + 4 * off, nullptr, 1, device, stream));
    }
    GSR_TRY(model_copy_back(os, out, dout, n_out, width));
    out->n = n_out;
    return os.finish();
}

extern "C" int32_t gsr_model_match(const gsr_model_view* a, const gsr_model_view* b, const gsr_fuse_params* params, int32_t* pairs,
                                   gsr_fuse_report* report, int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_model_match";
    if (const char* refused = match_check_args(a, b, params, report)) return fail(GSR_E_INVALID, "gsr_model_match: %s", refused);
    GSR_TRY(open_device(device, who));
    memset(report, 0, sizeof(*report));
    if (a->n + b->n == 0) return GSR_OK;

    FuseFront f;
    for (Event& e : f.ev) GSR_HIP(e.create());
    OneShot os((hipStream_t)stream, on_device != 0, who);
    size_t width[GSR_MODEL_NARR];
    bool used[GSR_MODEL_NARR];
    model_layout(0, false, width, used);                        // the search reads xyz, cov6, dc and opacity
    GSR_TRY(f.run(os, a, b, width, used, params, pairs));
    GSR_HIP(hipEventRecord(f.ev[3], os.st));
    GSR_TRY(f.counts(os, a->n, b->n, 3, report, pairs));
    return os.finish();
}
