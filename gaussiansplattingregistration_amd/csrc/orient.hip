// orient.hip -- consistent normal orientation on MI355X (gfx950), behind include/gsr_hip.h: Hoppe's
// propagation of a normal's sign along the minimum spanning forest of the neighbour graph, edge weight 1 - |n_i . n_j|.
//
//   gsr_orient_normals_graph   over given neighbour lists (the layout gsr_hybrid_search writes)
//   gsr_orient_normals         KDTreeSearchParamHybrid(radius, max_nn) lists through hybrid_search_dev, then the same
//
// The forest is Boruvka's, a lane per vertex, the union-find word of a vertex carrying its parity relative to its parent.  The
// steps are the functions of gsr_orient.h (which the host self-test runs serially); a kernel here is a grid-stride loop around one
// of them plus the wave-level counting.  Integer min / add atomics only: two runs give the same bits.  The host waits once for the
// number of CSR entries and once per round for the number of hooks; no kernel waits for another lane, and every in-kernel loop is
// bounded by its arguments.
#include "gsr_common.h"
#include "gsr_features.h"
#include "gsr_oneshot.h"
#include "gsr_orient.h"
#include "gsr_prims.h"

namespace gsr {

enum { ORIENT_CTR_FLIPPED = 0, ORIENT_CTR_ROOTS, ORIENT_CTR_NOT_LIVE, ORIENT_CTR_NOT_FLAT, ORIENT_CTR_HOOKS, ORIENT_NCTR = ORIENT_CTR_HOOKS + ORIENT_MAX_ROUNDS + 1 };

#define ORIENT_FOR_EACH_VERTEX(v) for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
// the same loop with every lane of the wave in every trip (the body votes with __ballot): `v < n` says whether the lane has a vertex
#define ORIENT_FOR_EACH_WAVE_TRIP(v) \
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, base_ = (int64_t)blockIdx.x * blockDim.x; base_ < n; \
         base_ += (int64_t)gridDim.x * blockDim.x, v += (int64_t)gridDim.x * blockDim.x)

__global__ __launch_bounds__(256) void k_orient_init(int64_t n, const double* __restrict__ nrm, uint8_t* __restrict__ live, uint32_t* __restrict__ par,
                                                     int* __restrict__ deg, int* __restrict__ cursor) {
    ORIENT_FOR_EACH_VERTEX(v) orient_init_vertex(v, nrm, live, par, deg, cursor);
    if (blockIdx.x == 0 && threadIdx.x == 0) deg[n] = 0;
}
__global__ __launch_bounds__(256) void k_orient_count(int64_t n, const int* __restrict__ nbr, int stride, const int* __restrict__ count,
                                                      const uint8_t* __restrict__ live, int* deg) {
    ORIENT_FOR_EACH_VERTEX(v) orient_count_vertex(v, n, nbr, stride, count, live, deg);
}
__global__ __launch_bounds__(256) void k_orient_fill(int64_t n, const int* __restrict__ nbr, int stride, const int* __restrict__ count,
                                                     const uint8_t* __restrict__ live, const double* __restrict__ nrm, const int* __restrict__ off, int* cursor,
                                                     int* adj, uint64_t* key) {
    ORIENT_FOR_EACH_VERTEX(v) orient_fill_vertex(v, n, nbr, stride, count, live, nrm, off, cursor, adj, key);
}
__global__ __launch_bounds__(256) void k_orient_min_weight(int64_t n, const uint32_t* __restrict__ par, const int* __restrict__ off, const int* __restrict__ adj,
                                                           const uint64_t* __restrict__ key, uint64_t* minw) {
    ORIENT_FOR_EACH_VERTEX(v) orient_min_weight_vertex(v, par, off, adj, key, minw);
}
__global__ __launch_bounds__(256) void k_orient_min_edge(int64_t n, const uint32_t* __restrict__ par, const int* __restrict__ off, const int* __restrict__ adj,
                                                         const uint64_t* __restrict__ key, const uint64_t* __restrict__ minw, uint64_t* minlohi) {
    ORIENT_FOR_EACH_VERTEX(v) orient_min_edge_vertex(v, par, off, adj, key, minw, minlohi);
}
__global__ __launch_bounds__(256) void k_orient_hook(int64_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const double* __restrict__ nrm,
                                                     const uint64_t* __restrict__ minw, const uint64_t* __restrict__ minlohi, int* hooks) {
    ORIENT_FOR_EACH_WAVE_TRIP(v) wave_count(v < n && orient_hook_vertex(v, in, out, nrm, minw, minlohi), hooks);
}
__global__ __launch_bounds__(256) void k_orient_jump(int64_t n, uint32_t* par) {
    ORIENT_FOR_EACH_VERTEX(v) orient_jump_vertex(v, par);
}
__global__ __launch_bounds__(256) void k_orient_check(int64_t n, const uint32_t* __restrict__ par, int* not_flat) {
    ORIENT_FOR_EACH_WAVE_TRIP(v) wave_count(v < n && !orient_is_flat(v, par), not_flat);
}
// the label of a component = its lowest vertex.  A wave whose lanes all sit in one component (the usual case once the forest is
// built) sends one min, its first lane's: one atomic per wave and destination, not 64 on one address.
__global__ __launch_bounds__(256) void k_orient_label(int64_t n, const uint32_t* __restrict__ par, int* label) {
    ORIENT_FOR_EACH_WAVE_TRIP(v) {
        const bool has = v < n;
        const uint32_t r = has ? (par[v] & ORIENT_PARENT) : 0u;
        const unsigned long long m = __ballot(has);
        if (!m) continue;
        const int first = __ffsll((long long)m) - 1;
        const uint32_t r0 = (uint32_t)__shfl((int)r, first);
        const bool uniform = __ballot(has && r != r0) == 0ull;
        if (has && (!uniform || (int)(threadIdx.x & 63) == first)) ORIENT_MIN_I32(&label[r], v);
    }
}
__global__ __launch_bounds__(256) void k_orient_vote(int64_t n, const uint32_t* __restrict__ par, const int* __restrict__ label, const uint8_t* __restrict__ live,
                                                     const float* __restrict__ xyz, const double* __restrict__ nrm, double cx, double cy, double cz, int* toward,
                                                     int* away) {
    ORIENT_FOR_EACH_WAVE_TRIP(v) {
        const bool has = v < n;
        const int t = has ? orient_vote_vertex(v, par, label, live, xyz, nrm, cx, cy, cz) : 0;
        const uint32_t r = has ? (par[v] & ORIENT_PARENT) : 0u;
        const unsigned long long m = __ballot(t != 0);
        if (!m) continue;
        const int first = __ffsll((long long)m) - 1;
        const uint32_t r0 = (uint32_t)__shfl((int)r, first);
        if (__ballot(t != 0 && r != r0) == 0ull) {                    // one component: two adds for the wave
            const int up = __popcll(__ballot(t > 0)), down = __popcll(__ballot(t < 0));
            if ((int)(threadIdx.x & 63) == first) {
                if (up) atomicAdd(&toward[r], up);
                if (down) atomicAdd(&away[r], down);
            }
        } else if (t != 0) {
            atomicAdd(t > 0 ? &toward[r] : &away[r], 1);
        }
    }
}
__global__ __launch_bounds__(256) void k_orient_flip(int64_t n, const uint32_t* __restrict__ par, const int* __restrict__ label, const uint8_t* __restrict__ live,
                                                     const int* __restrict__ toward, const int* __restrict__ away, int vote, double* nrm, int* component,
                                                     int* ctr) {
    ORIENT_FOR_EACH_WAVE_TRIP(v) {
        const int what = v < n ? orient_flip_vertex(v, par, label, live, toward, away, vote != 0, nrm, component) : 0;
        wave_count(what & ORIENT_IS_FLIPPED, ctr + ORIENT_CTR_FLIPPED);
        wave_count(what & ORIENT_IS_ROOT, ctr + ORIENT_CTR_ROOTS);
        wave_count(what & ORIENT_IS_NOT_LIVE, ctr + ORIENT_CTR_NOT_LIVE);
    }
}

namespace {

struct OrientHost {                      // what the read-backs land in: declared before the OneShot that waits for them
    int32_t entries;
    int32_t ctr[ORIENT_NCTR];
};

// the call behind both entry points, all pointers on the device; ev[1] .. ev[4] are recorded here
int32_t orient_run(OneShot& os, DevBuf& tmp_scan, Event* ev, OrientHost* host, size_t* workspace, const float* xyz, double* nrm, int64_t n, const int* nbr,
                   int32_t stride, const int* count, const double* reference, int32_t* component, gsr_orient_report* report) {
    hipStream_t st = os.st;
    const char* who = os.who;
    auto ws = [&](size_t bytes, auto** p) { *workspace += bytes; return os.scratch(bytes, p); };
    const size_t un = (size_t)n;
    const dim3 grid(stride_grid(n)), blk(256);
    uint8_t* live;
    uint32_t *par, *par2;
    int *deg, *off, *cursor, *label, *toward, *away, *ctr, *adj;
    uint64_t *minw, *key;                                             // minw[n] then minlohi[n]: one fill for both
    GSR_TRY(ws(un + 8, &live)); GSR_TRY(ws(un * 4 + 8, &par)); GSR_TRY(ws(un * 4 + 8, &par2)); GSR_TRY(ws((un + 1) * 4, &deg));
    GSR_TRY(ws((un + 1) * 4, &off)); GSR_TRY(ws(un * 4 + 8, &cursor)); GSR_TRY(ws(un * 4 + 8, &label)); GSR_TRY(ws(un * 8 + 8, &toward));
    GSR_TRY(ws(ORIENT_NCTR * 4, &ctr)); GSR_TRY(ws(un * 16 + 8, &minw));
    away = toward + n;
    uint64_t* minlohi = minw + n;
    GSR_HIP(hipMemsetAsync(ctr, 0, ORIENT_NCTR * 4, st));
    GSR_HIP(hipMemsetAsync(toward, 0, un * 8, st));
    GSR_HIP(hipMemsetAsync(label, 0x7f, un * 4, st));                 // 0x7f7f7f7f: above every index

    // ---- the symmetric CSR with its weights
    hipLaunchKernelGGL(k_orient_init, grid, blk, 0, st, n, (const double*)nrm, live, par, deg, cursor);
    hipLaunchKernelGGL(k_orient_count, grid, blk, 0, st, n, nbr, stride, count, (const uint8_t*)live, deg);
    GSR_TRY(scan_exclusive<rocprim::default_config>(tmp_scan, st, (const int*)deg, off, un + 1));
    GSR_HIP(hipMemcpyAsync(&host->entries, off + n, 4, hipMemcpyDeviceToHost, st));
    GSR_TRY(os.wait());
    const size_t entries = (size_t)host->entries;                     // <= 2 n stride < 2^31 (orient_check_args)
    GSR_TRY(ws(entries * 4 + 8, &adj)); GSR_TRY(ws(entries * 8 + 8, &key));
    hipLaunchKernelGGL(k_orient_fill, grid, blk, 0, st, n, nbr, stride, count, (const uint8_t*)live, (const double*)nrm, (const int*)off, cursor, adj, key);

    // ---- the rounds
    GSR_HIP(hipEventRecord(ev[2], st));
    const int launches = orient_jump_launches(n);
    int rounds = 0;
    for (;; ++rounds) {
        if (rounds == ORIENT_MAX_ROUNDS) return fail(GSR_E_HIP, "%s: the forest still grows after %d rounds (at most 31 are possible)", who, rounds);
        GSR_HIP(hipMemsetAsync(minw, 0xff, un * 16, st));
        hipLaunchKernelGGL(k_orient_min_weight, grid, blk, 0, st, n, (const uint32_t*)par, (const int*)off, (const int*)adj, (const uint64_t*)key, minw);
        hipLaunchKernelGGL(k_orient_min_edge, grid, blk, 0, st, n, (const uint32_t*)par, (const int*)off, (const int*)adj, (const uint64_t*)key,
                           (const uint64_t*)minw, minlohi);
        hipLaunchKernelGGL(k_orient_hook, grid, blk, 0, st, n, (const uint32_t*)par, par2, (const double*)nrm, (const uint64_t*)minw, (const uint64_t*)minlohi,
                           ctr + ORIENT_CTR_HOOKS + rounds);
        GSR_HIP(hipMemcpyAsync(host->ctr, ctr, sizeof(host->ctr), hipMemcpyDeviceToHost, st));
        GSR_TRY(os.wait());
        if (host->ctr[ORIENT_CTR_NOT_FLAT]) return fail(GSR_E_HIP, "%s: %d vertices do not reach a root after round %d", who, host->ctr[ORIENT_CTR_NOT_FLAT], rounds);
        if (host->ctr[ORIENT_CTR_HOOKS + rounds] == 0) break;          // (par2 == par: nothing hooked)
        for (int l = 0; l < launches; ++l) hipLaunchKernelGGL(k_orient_jump, grid, blk, 0, st, n, par2);
        hipLaunchKernelGGL(k_orient_check, grid, blk, 0, st, n, (const uint32_t*)par2, ctr + ORIENT_CTR_NOT_FLAT);
        uint32_t* t = par; par = par2; par2 = t;
    }

    // ---- labels, vote, flip
    GSR_HIP(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_orient_label, grid, blk, 0, st, n, (const uint32_t*)par, label);
    if (reference)
        hipLaunchKernelGGL(k_orient_vote, grid, blk, 0, st, n, (const uint32_t*)par, (const int*)label, (const uint8_t*)live, xyz, (const double*)nrm,
                           reference[0], reference[1], reference[2], toward, away);
    hipLaunchKernelGGL(k_orient_flip, grid, blk, 0, st, n, (const uint32_t*)par, (const int*)label, (const uint8_t*)live, (const int*)toward, (const int*)away,
                       reference ? 1 : 0, nrm, component, ctr);
    GSR_HIP(hipEventRecord(ev[4], st));
    GSR_HIP(hipMemcpyAsync(host->ctr, ctr, sizeof(host->ctr), hipMemcpyDeviceToHost, st));
    GSR_TRY(os.finish());
    report->n_components = host->ctr[ORIENT_CTR_ROOTS];
    report->n_flipped = host->ctr[ORIENT_CTR_FLIPPED];
    report->n_not_live = host->ctr[ORIENT_CTR_NOT_LIVE];
    report->rounds = rounds;
    report->workspace_bytes = (int64_t)*workspace;
    for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&report->phase_ms[k], ev[k], ev[k + 1]);
    return GSR_OK;
}

// radius < 0: the lists are the caller's; otherwise hybrid (radius, stride) lists are searched first
int32_t orient_call(const char* who, const float* xyz, double* normals, int64_t n, const int32_t* nbr, int32_t stride, const int32_t* count, double radius,
                    const double* reference, int32_t* component, gsr_orient_report* report, int32_t on_device, int32_t device, void* stream) {
    gsr_orient_report local;
    if (!report) report = &local;
    memset(report, 0, sizeof(*report));
    report->n = n;
    if (n == 0) return GSR_OK;
    GSR_TRY(open_device(device, who));
    Event ev[5];
    for (Event& e : ev) GSR_HIP(e.create());
    OrientHost host;
    DevBuf tmp_scan;                                                   // rocPRIM's temporary: freed after the OneShot's wait
    size_t workspace = 0;
    const size_t un = (size_t)n;
    OneShot os((hipStream_t)stream, on_device != 0, who);
    const float* dxyz = nullptr;
    const int *dnbr = nullptr, *dcnt = nullptr;
    double* dnrm = nullptr;
    int32_t* dcomp = nullptr;
    GSR_TRY(os.in(xyz, un * 12, &dxyz));
    GSR_TRY(os.out(normals, un * 24, &dnrm));
    if (!os.on_device) GSR_HIP(hipMemcpyAsync(dnrm, normals, un * 24, hipMemcpyHostToDevice, os.st));
    GSR_TRY(os.out(component, un * 4, &dcomp));
    if (!os.on_device) workspace += (xyz ? un * 12 : 0) + un * 24 + (component ? un * 4 : 0);
    GSR_HIP(hipEventRecord(ev[0], os.st));
    if (radius < 0.0) {
        GSR_TRY(os.in(nbr, un * (size_t)stride * 4, &dnbr));
        GSR_TRY(os.in(count, un * 4, &dcnt));
        if (!os.on_device) workspace += un * (size_t)stride * 4 + un * 4;
    } else {
        int *lists, *lens;
        GSR_TRY(os.scratch(un * (size_t)stride * 4, &lists)); GSR_TRY(os.scratch(un * 4, &lens));
        workspace += un * (size_t)stride * 4 + un * 4;
        GSR_TRY(hybrid_search_dev(dxyz, n, radius, stride, device, os.st, lists, lens));
        dnbr = lists; dcnt = lens;
    }
    GSR_HIP(hipEventRecord(ev[1], os.st));
    return orient_run(os, tmp_scan, ev, &host, &workspace, dxyz, dnrm, n, dnbr, stride, dcnt, reference, dcomp, report);
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" int32_t gsr_orient_normals_graph(const float* xyz, double* normals, int64_t n, const int32_t* nbr, int32_t stride, const int32_t* count,
                                            const double* reference, int32_t* component, gsr_orient_report* report, int32_t on_device, int32_t device,
                                            void* stream) {
    const char* who = "gsr_orient_normals_graph";
    if (const char* why = orient_check_args(xyz, normals, n, nbr, stride, count, reference)) return fail(GSR_E_INVALID, "%s: %s", who, why);
    return orient_call(who, xyz, normals, n, nbr, stride, count, -1.0, reference, component, report, on_device, device, stream);
}

extern "C" int32_t gsr_orient_normals(const float* xyz, double* normals, int64_t n, double radius, int32_t max_nn, const double* reference,
                                      int32_t* component, gsr_orient_report* report, int32_t on_device, int32_t device, void* stream) {
    const char* who = "gsr_orient_normals";
    if (!(radius > 0.0) || !__builtin_isfinite(radius)) return fail(GSR_E_INVALID, "%s: radius must be finite and > 0", who);
    if (max_nn < 1 || max_nn > GSR_HYBRID_MAX_NN) return fail(GSR_E_INVALID, "%s: max_nn must lie in [1, %d] (got %d)", who, GSR_HYBRID_MAX_NN, max_nn);
    const int32_t none = 0;                                            // the lists are made here: stand-ins for the NULL test
    if (const char* why = orient_check_args(xyz, normals, n, &none, max_nn, &none, reference)) return fail(GSR_E_INVALID, "%s: %s", who, why);
    if (n > 0 && !xyz) return fail(GSR_E_INVALID, "%s: xyz is required", who);
    return orient_call(who, xyz, normals, n, nullptr, max_nn, nullptr, radius, reference, component, report, on_device, device, stream);
}
