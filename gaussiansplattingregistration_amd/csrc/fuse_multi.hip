// fuse_multi.hip -- overlap-aware merge of N registered splat models in one pass (gsr_fuse_multi, include/gsr_hip.h; DESIGN.md
// section 20).  The definition is restated in float64 NumPy in tests/fuse_multi_model.py.
//
// Rows carry a GLOBAL index g, model-major.  Validity, the three gates and J are section 16's (gsr_fuse_dev.h); a GROUP holds at most
// one splat per model and is replaced by the moment-matched union of its members, everything else is copied bit for bit.
//
//   union copies       xyz, cov6, dc, opacity of the N models laid end to end (what the pre-pass, the grid and the search read);
//                      sh, scaling and rot stay where they are and are reached through a table of pointers (FmTable) by the writer
//   k_fuse_prep, k_fuse_moments / k_fuse_box, k_fuse_keys, sort, k_fuse_cell_starts      section 16's, over the union
//   k_fm_gather        the search arrays in cell order, the model id beside them
//   k_fm_search        a thread per row in cell order: 9 spans of <= 3 x-adjacent cells, same-model candidates leave on the xyz read,
//                      gates cheapest first; the running minima best[i][m] = (J32 bits << 32 | j) live in the thread's own LDS column
//                      (n_models x 256 x 8 B, no register array under a runtime index) and go to the thread's own row of the table:
//                      NO atomics
//   k_fm_mutual, scan, k_fm_edges    slot (i, m) holds a mutual edge iff i < j = best[i][m] and best[j][model(i)] = i; the compact
//                      list is in ascending (i, j) order, so the edge index orders like the tail of the key (J32, i, j)
//   rounds             k_fm_pick (a thread per live edge: 64-bit integer atomicMin of (J32 bits << 32 | edge) into the pick of both
//                      components), k_fm_merge (an edge both components picked merges them: a component merges at most once per
//                      round, so nobody else touches the two), k_fm_relabel (one hop).  The host reads the merge count per round.
//   k_fm_flags, scan x2, k_fm_members, k_fm_rows     group ranks, the rank x N member table addressed by model id, then a lane per
//                      output FLOAT: copied rows as 32-bit words, fused values as float64 sums in ascending member order
// One stream; the kernel boundary is the only synchronisation; no float atomics anywhere.
#include "gsr_common.h"
#include "gsr_oneshot.h"
#include "gsr_fuse_dev.h"
#include "gsr_fuse_args.h"
#include "gsr_prims.h"

#include <float.h>
#include <math.h>
#include <string.h>

namespace gsr {

#define FM_NONE (~0ull)

// where the rows of every model live: p[array][model] (NULL: the array is not carried), off[m] = the global index of model m's row 0
struct FmTable {
    const float* p[GSR_MODEL_NARR][GSR_FUSE_MAX_MODELS];
    int64_t off[GSR_FUSE_MAX_MODELS + 1];
};

// the union's search arrays in cell order; an invalid splat gets NaN centres, which fail the distance gate
__global__ __launch_bounds__(256) void k_fm_gather(int64_t n, const unsigned* __restrict__ order, const float* __restrict__ xyz, const float* __restrict__ dc,
                                                   const float* __restrict__ cov6, const double* __restrict__ w, const double* __restrict__ inv,
                                                   const uint8_t* __restrict__ model, float* __restrict__ sxyz, float* __restrict__ sdc,
                                                   float* __restrict__ scov, double* __restrict__ sinv, uint8_t* __restrict__ smodel) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = order[p];
        const bool valid = w[a] > 0.0;
        const float nan = __builtin_nanf("");
        for (int k = 0; k < 3; ++k) { sxyz[3 * p + k] = valid ? xyz[3 * a + k] : nan; sdc[3 * p + k] = dc[3 * a + k]; }
        for (int k = 0; k < 6; ++k) { scov[6 * p + k] = cov6[6 * a + k]; sinv[6 * p + k] = inv[6 * a + k]; }
        smodel[p] = model[a];
    }
}

// best[i][m] of every row: the thread's own column of LDS holds the running minima, nothing is shared between threads
__global__ __launch_bounds__(256) void k_fm_search(int64_t n, int N, const unsigned* __restrict__ order, const FuseGrid* __restrict__ G,
                                                   const int* __restrict__ cellStart, const float* __restrict__ sxyz, const float* __restrict__ sdc,
                                                   const float* __restrict__ scov, const double* __restrict__ sinv, const uint8_t* __restrict__ smodel,
                                                   double r2, double kld_max, double cd2, unsigned long long* __restrict__ best,
                                                   unsigned long long* __restrict__ n_gated) {
    extern __shared__ unsigned long long fm_min[];              // [m * 256 + thread]
    const FuseGrid g = *G;
    unsigned gated = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        for (int m = 0; m < N; ++m) fm_min[m * 256 + threadIdx.x] = FM_NONE;
        const unsigned me = order[t];
        const float fx = sxyz[3 * t], fy = sxyz[3 * t + 1], fz = sxyz[3 * t + 2];
        if (fx == fx) {                                          // valid (an invalid row carries NaN centres)
            const unsigned mine = smodel[t];
            const double bx = fx, by = fy, bz = fz;
            const double e0 = sdc[3 * t], e1 = sdc[3 * t + 1], e2 = sdc[3 * t + 2];
            double Mc[6], Mi[6];
            for (int k = 0; k < 6; ++k) { Mc[k] = scov[6 * t + k]; Mi[k] = sinv[6 * t + k]; }
            const int cx = fuse_cell(bx, g.ox, g.inv_c, g.gx), cy = fuse_cell(by, g.oy, g.inv_c, g.gy), cz = fuse_cell(bz, g.oz, g.inv_c, g.gz);
            const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.gx - 1 ? cx + 1 : g.gx - 1;
            const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < g.gy - 1 ? cy + 1 : g.gy - 1;
            const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < g.gz - 1 ? cz + 1 : g.gz - 1;
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.gy + y) * g.gx;
                    const int p1 = cellStart[row + x1 + 1];
                    for (int p = cellStart[row + x0]; p < p1; ++p) {
                        const unsigned cm = smodel[p];
                        if (cm == mine) continue;
                        // the sign of the difference does not reach the result: every term below is a product of two differences
                        const double dx = (double)sxyz[3 * (int64_t)p] - bx, dy = (double)sxyz[3 * (int64_t)p + 1] - by, dz = (double)sxyz[3 * (int64_t)p + 2] - bz;
                        if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
                        const double f0 = (double)sdc[3 * (int64_t)p] - e0, f1 = (double)sdc[3 * (int64_t)p + 1] - e1, f2 = (double)sdc[3 * (int64_t)p + 2] - e2;
                        if (!((f0 * f0 + f1 * f1) + f2 * f2 <= cd2)) continue;
                        double Cc[6], Ci[6];
                        for (int k = 0; k < 6; ++k) { Cc[k] = scov[6 * (int64_t)p + k]; Ci[k] = sinv[6 * (int64_t)p + k]; }
                        const unsigned c = order[p];
                        // section 16's expression with the LOWER global index as `a`.  Swapping the roles swaps the operands of the two
                        // inner additions and nothing else, and an IEEE addition commutes bit for bit: one form serves both ends of a
                        // pair, which therefore compute the same bits
                        double J = 0.25 * (((sym_trace(Mi, Cc) + sym_trace(Ci, Mc)) - 6.0) + (sym_quad(Ci, dx, dy, dz) + sym_quad(Mi, dx, dy, dz)));
                        if (J < 0.0) J = 0.0;                   // rounding only: J >= 0 in exact arithmetic
                        if (!(J <= kld_max)) continue;
                        const unsigned long long k = ((unsigned long long)__float_as_uint((float)J) << 32) | c;
                        unsigned long long* slot = &fm_min[cm * 256 + threadIdx.x];
                        if (k < *slot) *slot = k;
                        gated += c > me ? 1u : 0u;              // every pair once: at its lower end
                    }
                }
        }
        for (int m = 0; m < N; ++m) best[(int64_t)me * N + m] = fm_min[m * 256 + threadIdx.x];
    }
    for (int o = 32; o > 0; o >>= 1) gated += __shfl_xor(gated, o);
    if ((threadIdx.x & 63) == 0 && gated) atomicAdd(n_gated, (unsigned long long)gated);
}

// slot s = i * N + m holds a mutual edge iff j = best[i][m] exists, i < j and best[j][model(i)] = i; flag[slots] = 0 closes the scan
__global__ __launch_bounds__(256) void k_fm_mutual(int64_t slots, int N, const unsigned long long* __restrict__ best, const uint8_t* __restrict__ model,
                                                   int* __restrict__ flag) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= slots; s += (int64_t)gridDim.x * blockDim.x) {
        int f = 0;
        if (s < slots) {
            const unsigned long long k = best[s];
            const int64_t i = s / N;
            if (k != FM_NONE) {
                const int64_t j = (int64_t)(k & 0xffffffffull);
                if (i < j) {
                    const unsigned long long back = best[j * N + model[i]];
                    f = back != FM_NONE && (int64_t)(back & 0xffffffffull) == i;
                }
            }
        }
        flag[s] = f;
    }
}

__global__ __launch_bounds__(256) void k_fm_edges(int64_t slots, int N, const unsigned long long* __restrict__ best, const int* __restrict__ flag,
                                                  const int* __restrict__ scan, int* __restrict__ eu, int* __restrict__ ev, unsigned* __restrict__ ej,
                                                  uint8_t* __restrict__ alive) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x)
        if (flag[s]) {
            const unsigned long long k = best[s];
            const int e = scan[s];
            eu[e] = (int)(s / N); ev[e] = (int)(unsigned)(k & 0xffffffffull); ej[e] = (unsigned)(k >> 32); alive[e] = 1;
        }
}

__global__ __launch_bounds__(256) void k_fm_init(int64_t n, const uint8_t* __restrict__ model, int* __restrict__ label, int* __restrict__ parent,
                                                 unsigned* __restrict__ mask, unsigned long long* __restrict__ pick) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        label[i] = parent[i] = (int)i;
        mask[i] = 1u << model[i];
        pick[i] = FM_NONE;
    }
}

// counters: [0] rejected edges, [1] merges (cumulative)
__global__ __launch_bounds__(256) void k_fm_pick(int64_t ne, const int* __restrict__ eu, const int* __restrict__ ev, const unsigned* __restrict__ ej,
                                                 uint8_t* __restrict__ alive, const int* __restrict__ label, const unsigned* __restrict__ mask,
                                                 unsigned long long* __restrict__ pick, unsigned long long* __restrict__ counters) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        if (!alive[e]) continue;
        const int cu = label[eu[e]], cv = label[ev[e]];
        if (cu == cv) { alive[e] = 0; continue; }                                   // inside one component
        if (mask[cu] & mask[cv]) { alive[e] = 0; atomicAdd(&counters[0], 1ull); continue; }      // the union would hold two rows of a model
        const unsigned long long k = ((unsigned long long)ej[e] << 32) | (unsigned long long)e;
        atomicMin(&pick[cu], k);
        atomicMin(&pick[cv], k);
    }
}

// an edge that is the pick of both its components merges them; a component has one pick, so no other thread touches either
__global__ __launch_bounds__(256) void k_fm_merge(int64_t ne, const int* __restrict__ eu, const int* __restrict__ ev, const unsigned* __restrict__ ej,
                                                  uint8_t* __restrict__ alive, const int* __restrict__ label, unsigned* __restrict__ mask,
                                                  const unsigned long long* __restrict__ pick, int* __restrict__ parent, unsigned long long* __restrict__ counters) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        if (!alive[e]) continue;
        const int cu = label[eu[e]], cv = label[ev[e]];
        const unsigned long long k = ((unsigned long long)ej[e] << 32) | (unsigned long long)e;
        if (pick[cu] != k || pick[cv] != k) continue;
        const int lo = cu < cv ? cu : cv, hi = cu < cv ? cv : cu;
        parent[hi] = lo;
        mask[lo] = mask[lo] | mask[hi];
        alive[e] = 0;
        atomicAdd(&counters[1], 1ull);
    }
}

__global__ __launch_bounds__(256) void k_fm_relabel(int64_t n, int* __restrict__ label, const int* __restrict__ parent, unsigned long long* __restrict__ pick) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = label[i];
        label[i] = parent[l];                                   // one hop: the component `l` merged at most once this round
        pick[i] = FM_NONE;
    }
}

// grouped[i]: the row's group has >= 2 members; root[i]: it is the lowest of them.  hist[k]: the groups of k members, counted per block in
// LDS first (integer atomics): one global atomic per block and size, not one per group on 17 addresses.  Entry n of both flags = 0.
__global__ __launch_bounds__(256) void k_fm_flags(int64_t n, const int* __restrict__ label, const unsigned* __restrict__ mask, int* __restrict__ grouped,
                                                  int* __restrict__ root, unsigned long long* __restrict__ hist) {
    __shared__ unsigned h[GSR_FUSE_MAX_MODELS + 1];
    if (threadIdx.x <= GSR_FUSE_MAX_MODELS) h[threadIdx.x] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
        int gflag = 0, rflag = 0;
        if (i < n) {
            const int l = label[i];
            const int k = __popc(mask[l]);
            gflag = k >= 2;
            rflag = gflag && l == (int)i;
            if (rflag) atomicAdd(&h[k], 1u);
        }
        grouped[i] = gflag; root[i] = rflag;
    }
    __syncthreads();
    if (threadIdx.x <= GSR_FUSE_MAX_MODELS && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// member[rank * N + model] = the group's row of that model (the mask rule makes the slot unique); group_of for the caller
__global__ __launch_bounds__(256) void k_fm_members(int64_t n, int N, const int* __restrict__ label, const int* __restrict__ grouped, const int* __restrict__ scanR,
                                                    const int* __restrict__ scanG, const uint8_t* __restrict__ model, int* __restrict__ member,
                                                    int32_t* __restrict__ group_of) {
    const int64_t n_copied = n - scanG[n];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t go = -1;
        if (grouped[i]) {
            const int rank = scanR[label[i]];
            member[(int64_t)rank * N + model[i]] = (int)i;
            go = (int32_t)(n_copied + rank);
        }
        if (group_of) group_of[i] = go;
    }
}

// One array of the output, a lane per float of the union (consecutive lanes on consecutive addresses of a row).
//   a row in no group          its W words, copied as integers
//   the lowest row of a group  FM_MEAN: sum w v / sum w over the members in ascending order; FM_COV (W = 6): sum w (C + d d^T) / sum w,
//                              d = the member's centre minus the fused centre; float64, narrowed once; FM_COPY: left for gsr_decompose_cov
//   any other grouped row      nothing
#define FM_COPY 0
#define FM_MEAN 1
#define FM_COV 2
__global__ __launch_bounds__(256) void k_fm_rows(int64_t n, int N, int W, int mode, int arr, const FmTable* __restrict__ T, float* __restrict__ O,
                                                 const int* __restrict__ label, const int* __restrict__ grouped, const int* __restrict__ scanG,
                                                 const int* __restrict__ scanR, const int* __restrict__ member, const uint8_t* __restrict__ model,
                                                 const double* __restrict__ w, const float* __restrict__ xyz) {
    const int64_t total = n * W;
    const int64_t n_copied = n - scanG[n];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / W;
        const int j = (int)(t - i * W);
        if (!grouped[i]) {
            const int m = model[i];
            reinterpret_cast<uint32_t*>(O)[(i - scanG[i]) * W + j] = reinterpret_cast<const uint32_t*>(T->p[arr][m])[(i - T->off[m]) * W + j];
            continue;
        }
        if (mode == FM_COPY || label[i] != (int)i) continue;
        const int rank = scanR[i];
        const int* mem = member + (int64_t)rank * N;
        double ws = 0.0, v = 0.0;
        if (mode == FM_MEAN) {
            for (int m = 0; m < N; ++m) {
                const int64_t r = mem[m];
                if (r < 0) continue;
                ws += w[r];
                v += w[r] * (double)T->p[arr][m][(r - T->off[m]) * W + j];
            }
            v /= ws;
        } else {
            const int a = j < 3 ? 0 : j < 5 ? 1 : 2, b = j < 3 ? j : j < 5 ? j - 2 : 2;      // (xx, xy, xz, yy, yz, zz)
            double sa = 0.0, sb = 0.0;
            for (int m = 0; m < N; ++m) {
                const int64_t r = mem[m];
                if (r < 0) continue;
                ws += w[r];
                sa += w[r] * (double)xyz[3 * r + a];
                sb += w[r] * (double)xyz[3 * r + b];
            }
            const double ma = sa / ws, mb = sb / ws;
            for (int m = 0; m < N; ++m) {
                const int64_t r = mem[m];
                if (r < 0) continue;
                v += w[r] * ((double)T->p[arr][m][(r - T->off[m]) * W + j] + ((double)xyz[3 * r + a] - ma) * ((double)xyz[3 * r + b] - mb));
            }
            v /= ws;
        }
        O[(n_copied + rank) * W + j] = (float)v;
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_fuse_multi(const gsr_model_view* models, int32_t n_models, int32_t K, const gsr_fuse_params* params, gsr_model_view* out,
                                        int32_t* group_of, gsr_fuse_multi_report* report, int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_fuse_multi";
    int64_t off[GSR_FUSE_MAX_MODELS + 1];
    size_t width[GSR_MODEL_NARR];
    bool used[GSR_MODEL_NARR], with_sr = false;
    char why[256];
    if (const char* refused = fuse_multi_check_args(models, n_models, K, params, out, group_of, report, off, width, used, &with_sr, why, sizeof why))
        return fail(GSR_E_INVALID, "gsr_fuse_multi: %s", refused);
    const int N = n_models;
    const int64_t n = off[N];
    const int modes[GSR_MODEL_NARR] = {FM_MEAN, FM_COV, FM_MEAN, FM_MEAN, FM_MEAN, FM_COPY, FM_COPY};
    memset(report, 0, sizeof(*report));
    GSR_TRY(open_device(device, who));
    if (n == 0) { out->n = 0; return GSR_OK; }

    const bool dev = on_device != 0;
    DevBuf tmp_sort, tmp_scan_e, tmp_scan_g, tmp_scan_r;       // rocPRIM's temporaries: declared before the OneShot, freed after its wait
    FmTable tab;                                                // (copied to the device asynchronously: lives until the OneShot's wait too)
    memset(&tab, 0, sizeof(tab));
    Event ev[6];
    for (Event& e : ev) GSR_HIP(e.create());
    OneShot os((hipStream_t)stream, dev, who);
    hipStream_t st = os.st;
    size_t workspace = 0;
    auto ws = [&](size_t bytes, auto** p) { workspace += bytes; return os.scratch(bytes, p); };
    const size_t un = (size_t)n;

    // ---- the union copies of the arrays the search reads, the table of the others
    float* uni[GSR_MODEL_NARR] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* dout[GSR_MODEL_NARR];
    for (int k = 0; k < GSR_MODEL_NARR; ++k) {
        if (!used[k]) continue;
        const bool in_union = k == 0 || k == 1 || k == 2 || k == 4;
        if (in_union) GSR_TRY(ws(un * width[k] * 4 + 8, &uni[k]));
        for (int m = 0; m < N; ++m) {
            const int64_t nm = models[m].n;
            if (nm == 0) continue;
            const float* src = model_array(models + m, k);
            if (in_union) {
                float* dst = uni[k] + (size_t)off[m] * width[k];
                GSR_HIP(hipMemcpyAsync(dst, src, (size_t)nm * width[k] * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
                tab.p[k][m] = dst;
            } else {
                GSR_TRY(os.in(src, (size_t)nm * width[k] * 4, &tab.p[k][m]));
            }
        }
    }
    GSR_TRY(model_out(os, out, n, width, used, dout));
    for (int m = 0; m <= GSR_FUSE_MAX_MODELS; ++m) tab.off[m] = off[m <= N ? m : N];
    int32_t* dgroup = nullptr;
    if (group_of) { if (dev) dgroup = group_of; else GSR_TRY(os.scratch(un * 4, &dgroup)); }

    FmTable* dtab;
    uint8_t *model, *smodel;
    double *w, *inv, *sinv;
    float *sxyz, *sdc, *scov;
    unsigned* mask;
    int *eflag, *escan, *label, *parent, *grouped, *root, *scanG, *scanR;
    unsigned long long *best, *pick, *counters;                 // counters: [0] rejected, [1] merges, [2] invalid, [3] gated, [4 ..] histogram
    FuseCells c;
    const int64_t slots = n * N;
    const size_t us = (size_t)slots;
    const int NCOUNT = 4 + GSR_FUSE_MAX_MODELS + 1;
    GSR_TRY(ws(sizeof(FmTable), &dtab));
    GSR_TRY(ws(un + 8, &model)); GSR_TRY(ws(un + 8, &smodel));
    GSR_TRY(ws(un * 8 + 8, &w)); GSR_TRY(ws(un * 48 + 8, &inv));
    GSR_TRY(ws(un * 48 + 8, &sinv)); GSR_TRY(ws(un * 12 + 8, &sxyz)); GSR_TRY(ws(un * 12 + 8, &sdc)); GSR_TRY(ws(un * 24 + 8, &scov));
    GSR_TRY(ws(us * 8 + 8, &best));
    GSR_TRY(ws((us + 1) * 4, &eflag)); GSR_TRY(ws((us + 1) * 4, &escan));
    GSR_TRY(ws(un * 4 + 8, &label)); GSR_TRY(ws(un * 4 + 8, &parent)); GSR_TRY(ws(un * 4 + 8, &mask)); GSR_TRY(ws(un * 8 + 8, &pick));
    GSR_TRY(ws((un + 1) * 4, &grouped)); GSR_TRY(ws((un + 1) * 4, &root)); GSR_TRY(ws((un + 1) * 4, &scanG)); GSR_TRY(ws((un + 1) * 4, &scanR));
    GSR_TRY(ws((size_t)NCOUNT * 8, &counters));
    GSR_TRY(c.reserve(os, workspace, n));
    GSR_HIP(hipMemcpyAsync(dtab, &tab, sizeof(tab), hipMemcpyHostToDevice, st));
    GSR_HIP(hipMemsetAsync(counters, 0, (size_t)NCOUNT * 8, st));
    for (int m = 0; m < N; ++m)
        if (models[m].n > 0) GSR_HIP(hipMemsetAsync(model + off[m], m, (size_t)models[m].n, st));

    // ---- pre-pass and grid
    GSR_HIP(hipEventRecord(ev[0], st));
    GSR_TRY(c.launch(st, tmp_sort, uni[0], uni[1], uni[4], w, inv, counters + 2, params->max_distance));
    hipLaunchKernelGGL(k_fm_gather, dim3(stride_grid(n)), dim3(256), 0, st, n, (const unsigned*)c.order, (const float*)uni[0], (const float*)uni[2], (const float*)uni[1],
                       (const double*)w, (const double*)inv, (const uint8_t*)model, sxyz, sdc, scov, sinv, smodel);
    // ---- search
    GSR_HIP(hipEventRecord(ev[1], st));
    const double r2 = params->max_distance * params->max_distance, cd2 = params->color_delta * params->color_delta;
    hipLaunchKernelGGL(k_fm_search, dim3(stride_grid(n)), dim3(256), (size_t)N * 256 * 8, st, n, N, (const unsigned*)c.order, (const FuseGrid*)c.grid, (const int*)c.cellStart,
                       (const float*)sxyz, (const float*)sdc, (const float*)scov, (const double*)sinv, (const uint8_t*)smodel, r2, params->kld_max, cd2, best, counters + 3);
    // ---- the edge list
    GSR_HIP(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_fm_mutual, dim3(stride_grid(slots + 1)), dim3(256), 0, st, slots, N, (const unsigned long long*)best, (const uint8_t*)model, eflag);
    GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan_e, st, (const int*)eflag, escan, us + 1));
    int h_edges = 0;
    GSR_HIP(hipMemcpyAsync(&h_edges, escan + slots, 4, hipMemcpyDeviceToHost, st));
    GSR_TRY(os.wait());                                         // the edge count sizes the list
    const int64_t ne = h_edges;
    int *eu = nullptr, *evx = nullptr;
    unsigned* ej = nullptr;
    uint8_t* alive = nullptr;
    GSR_TRY(ws((size_t)ne * 4 + 8, &eu)); GSR_TRY(ws((size_t)ne * 4 + 8, &evx)); GSR_TRY(ws((size_t)ne * 4 + 8, &ej)); GSR_TRY(ws((size_t)ne + 8, &alive));
    if (ne > 0)
        hipLaunchKernelGGL(k_fm_edges, dim3(stride_grid(slots)), dim3(256), 0, st, slots, N, (const unsigned long long*)best, (const int*)eflag, (const int*)escan, eu, evx,
                           ej, alive);
    hipLaunchKernelGGL(k_fm_init, dim3(stride_grid(n)), dim3(256), 0, st, n, (const uint8_t*)model, label, parent, mask, pick);
    // ---- rounds: until one merges nothing (a round with a live edge merges at least the globally smallest one)
    GSR_HIP(hipEventRecord(ev[3], st));
    int64_t rounds = 0;
    unsigned long long hrm[2] = {0, 0}, merged_before = 0;
    while (ne > 0) {
        hipLaunchKernelGGL(k_fm_pick, dim3(stride_grid(ne)), dim3(256), 0, st, ne, (const int*)eu, (const int*)evx, (const unsigned*)ej, alive, (const int*)label,
                           (const unsigned*)mask, pick, counters);
        hipLaunchKernelGGL(k_fm_merge, dim3(stride_grid(ne)), dim3(256), 0, st, ne, (const int*)eu, (const int*)evx, (const unsigned*)ej, alive, (const int*)label, mask,
                           (const unsigned long long*)pick, parent, counters);
        hipLaunchKernelGGL(k_fm_relabel, dim3(stride_grid(n)), dim3(256), 0, st, n, label, (const int*)parent, pick);
        GSR_HIP(hipMemcpyAsync(hrm, counters, sizeof(hrm), hipMemcpyDeviceToHost, st));
        GSR_TRY(os.wait());
        if (hrm[1] == merged_before) break;
        merged_before = hrm[1];
        ++rounds;
        if (rounds > ne) return fail(GSR_E_HIP, "gsr_fuse_multi: the rounds do not end");      // (cannot happen: every counted round merges)
    }
    // ---- group ranks
    GSR_HIP(hipEventRecord(ev[4], st));
    hipLaunchKernelGGL(k_fm_flags, dim3(stride_grid(n + 1)), dim3(256), 0, st, n, (const int*)label, (const unsigned*)mask, grouped, root, counters + 4);
    GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan_g, st, (const int*)grouped, scanG, un + 1));
    GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan_r, st, (const int*)root, scanR, un + 1));
    unsigned long long hc[4 + GSR_FUSE_MAX_MODELS + 1];
    int h_grouped = 0, h_groups = 0;
    GSR_HIP(hipMemcpyAsync(hc, counters, sizeof(hc), hipMemcpyDeviceToHost, st));
    GSR_HIP(hipMemcpyAsync(&h_grouped, scanG + n, 4, hipMemcpyDeviceToHost, st));
    GSR_HIP(hipMemcpyAsync(&h_groups, scanR + n, 4, hipMemcpyDeviceToHost, st));
    GSR_TRY(os.wait());                                         // the group count sizes the member table
    const int64_t ng = h_groups, n_copied = n - h_grouped, n_out = n_copied + ng;
    int* member = nullptr;
    GSR_TRY(ws((size_t)ng * N * 4 + 8, &member));
    GSR_HIP(hipMemsetAsync(member, 0xff, (size_t)ng * N * 4 + 8, st));
    hipLaunchKernelGGL(k_fm_members, dim3(stride_grid(n)), dim3(256), 0, st, n, N, (const int*)label, (const int*)grouped, (const int*)scanR, (const int*)scanG,
                       (const uint8_t*)model, member, dgroup);
    // ---- writer
    for (int k = 0; k < GSR_MODEL_NARR; ++k)
        if (used[k])
            hipLaunchKernelGGL(k_fm_rows, dim3(stride_grid(n * (int64_t)width[k])), dim3(256), 0, st, n, N, (int)width[k], modes[k], k, (const FmTable*)dtab, dout[k],
                               (const int*)label, (const int*)grouped, (const int*)scanG, (const int*)scanR, (const int*)member, (const uint8_t*)model, (const double*)w,
                               (const float*)uni[0]);
    GSR_HIP(hipEventRecord(ev[5], st));
    GSR_TRY(os.wait());
    report->n_out = n_out; report->n_groups = ng; report->n_grouped_rows = h_grouped;
    report->n_invalid = (int64_t)hc[2]; report->gated_pairs = (int64_t)hc[3]; report->mutual_edges = ne; report->rejected_edges = (int64_t)hc[0];
    report->rounds = rounds;
    for (int k = 0; k <= GSR_FUSE_MAX_MODELS; ++k) report->groups_of_size[k] = (int64_t)hc[4 + k];
    for (int k = 0; k < 5; ++k) (void)hipEventElapsedTime(&report->phase_ms[k], ev[k], ev[k + 1]);
    report->workspace_bytes = (int64_t)(workspace + tmp_sort.cap + tmp_scan_e.cap + tmp_scan_g.cap + tmp_scan_r.cap);
    if (with_sr && ng > 0)
        GSR_TRY(gsr_decompose_cov(dout[1] + 6 * n_copied, ng, GSR_DECOMP_EXACT, dout[5] + 3 * n_copied, dout[6] + 4 * n_copied, nullptr, 1, device, stream));
    GSR_TRY(model_copy_back(os, out, dout, n_out, width));
    if (!dev && dgroup) GSR_HIP(hipMemcpyAsync(group_of, dgroup, un * 4, hipMemcpyDeviceToHost, st));
    out->n = n_out;
    return os.finish();
}

// The same entry point under the name the pairwise one suggests (gsr_model_fuse + _multi), for callers that look it up by that name.
// include/gsr_hip.h and the Python binding table declare gsr_fuse_multi only.
extern "C" int32_t gsr_model_fuse_multi(const gsr_model_view* models, int32_t n_models, int32_t K, const gsr_fuse_params* params, gsr_model_view* out,
                                        int32_t* group_of, gsr_fuse_multi_report* report, int32_t on_device, int32_t device, void* stream) {
    return gsr_fuse_multi(models, n_models, K, params, out, group_of, report, on_device, device, stream);
}
