// gsr_orient.h -- consistent normal orientation: the per-item steps of a Boruvka minimum spanning forest
// with a parity bit in the union-find, over plain arrays.  No HIP runtime here: csrc/orient.hip calls each step from a kernel, a
// lane per item, and scripts/orient_selftest.cpp calls the same steps serially under the host sanitizers.  The only thing that
// differs between the two is the shim below (integer min / add on one word: atomic on the device, plain on the host).
//
// Every loop in this file has a trip count bounded by its arguments: a row of `stride` entries, an adjacency of off[v + 1] - off[v]
// entries, a parent walk of ORIENT_JUMPS hops.  None waits for another lane.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define ORIENT_MIN_U64(p, v) ((void)atomicMin((unsigned long long*)(p), (unsigned long long)(v)))
#define ORIENT_MIN_I32(p, v) ((void)atomicMin((int*)(p), (int)(v)))
#define ORIENT_ADD_I32(p, v) atomicAdd((int*)(p), (int)(v))
#else
#define ORIENT_MIN_U64(p, v) ((void)(*(p) = (uint64_t)(v) < *(p) ? (uint64_t)(v) : *(p)))
#define ORIENT_MIN_I32(p, v) ((void)(*(p) = (int32_t)(v) < *(p) ? (int32_t)(v) : *(p)))
#define ORIENT_ADD_I32(p, v) orient_host_add(p, v)
inline int32_t orient_host_add(int32_t* p, int32_t v) { const int32_t old = *p; *p = old + v; return old; }
#endif

namespace gsr {

#define ORIENT_NONE 0xFFFFFFFFFFFFFFFFull      // no candidate yet (minw, minlohi)
#define ORIENT_KEY_NAN 0xFFFFFFFFFFFFFFFEull   // a NaN weight (overflowing normals): after every number, before "none"
#define ORIENT_PARENT 0x7FFFFFFFu              // word = parent index | parity relative to the parent << 31
#define ORIENT_JUMPS 32                        // hops of one parent walk; ORIENT_JUMPS^launches >= n bounds the launches of a round
#define ORIENT_MAX_ROUNDS 32                   // Boruvka halves the components: 31 rounds for n < 2^31, the 32nd is an error

// what the flip step says about a vertex (the kernel counts them)
#define ORIENT_IS_FLIPPED 1
#define ORIENT_IS_ROOT 2
#define ORIENT_IS_NOT_LIVE 4

GSR_HD bool orient_finite3(double x, double y, double z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// dot = n_i . n_j, x then y then z (the build does not contract: NumPy's arithmetic bit for bit; symmetric in i and j)
GSR_HD double orient_dot(const double* nrm, int64_t i, int64_t j) {
    return nrm[i * 3] * nrm[j * 3] + nrm[i * 3 + 1] * nrm[j * 3 + 1] + nrm[i * 3 + 2] * nrm[j * 3 + 2];
}
// w = 1 - |dot| as an unsigned key of the same order (negative weights of non-unit normals included)
GSR_HD uint64_t orient_key(double dot) {
    const double w = 1.0 - __builtin_fabs(dot);
    if (w != w) return ORIENT_KEY_NAN;
    uint64_t b;
    __builtin_memcpy(&b, &w, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// entry k of row v, or -1 when it is skipped: the vertex itself, an index outside [0, n) (never dereferenced), a dead end
GSR_HD int32_t orient_entry(const int32_t* nbr, int32_t stride, int64_t n, const uint8_t* live, int64_t v, int32_t k) {
    const int32_t j = nbr[v * stride + k];
    if ((uint32_t)j >= (uint64_t)n || j == v || !live[j]) return -1;
    return j;
}
GSR_HD int32_t orient_row_len(const int32_t* count, int32_t stride, int64_t v) {
    const int32_t c = count[v];
    return c < 0 ? 0 : (c > stride ? stride : c);
}

// ---- the symmetric CSR: every directed entry (v, j) is stored with both ends ---------------------------------------------------
GSR_HD void orient_init_vertex(int64_t v, const double* nrm, uint8_t* live, uint32_t* par, int32_t* deg, int32_t* cursor) {
    live[v] = orient_finite3(nrm[v * 3], nrm[v * 3 + 1], nrm[v * 3 + 2]) ? 1 : 0;
    par[v] = (uint32_t)v;
    deg[v] = 0;
    cursor[v] = 0;
}
GSR_HD void orient_count_vertex(int64_t v, int64_t n, const int32_t* nbr, int32_t stride, const int32_t* count, const uint8_t* live, int32_t* deg) {
    if (!live[v]) return;
    const int32_t len = orient_row_len(count, stride, v);
    int32_t own = 0;
    for (int32_t k = 0; k < len; ++k) {
        const int32_t j = orient_entry(nbr, stride, n, live, v, k);
        if (j < 0) continue;
        ++own;
        (void)ORIENT_ADD_I32(&deg[j], 1);
    }
    if (own) (void)ORIENT_ADD_I32(&deg[v], own);
}
// off = exclusive scan of deg (n + 1 entries).  The order inside an adjacency depends on the arrival order; nothing below does.
GSR_HD void orient_fill_vertex(int64_t v, int64_t n, const int32_t* nbr, int32_t stride, const int32_t* count, const uint8_t* live, const double* nrm,
                               const int32_t* off, int32_t* cursor, int32_t* adj, uint64_t* key) {
    if (!live[v]) return;
    const int32_t len = orient_row_len(count, stride, v);
    for (int32_t k = 0; k < len; ++k) {
        const int32_t j = orient_entry(nbr, stride, n, live, v, k);
        if (j < 0) continue;
        const uint64_t w = orient_key(orient_dot(nrm, v, j));
        const int32_t a = off[v] + ORIENT_ADD_I32(&cursor[v], 1), b = off[j] + ORIENT_ADD_I32(&cursor[j], 1);
        if (a < off[v + 1]) { adj[a] = j; key[a] = w; }               // (always true: the count step saw the same entries)
        if (b < off[j + 1]) { adj[b] = (int32_t)v; key[b] = w; }
    }
}

// ---- one round -----------------------------------------------------------------------------------------------------------------
// Between rounds every word points at a root, so par[v] & ORIENT_PARENT is the component of v.
// (a1) the least weight among the edges that leave the component of v
GSR_HD void orient_min_weight_vertex(int64_t v, const uint32_t* par, const int32_t* off, const int32_t* adj, const uint64_t* key, uint64_t* minw) {
    const uint32_t r = par[v] & ORIENT_PARENT;
    uint64_t best = ORIENT_NONE;
    for (int32_t e = off[v]; e < off[v + 1]; ++e)
        if ((par[adj[e]] & ORIENT_PARENT) != r && key[e] < best) best = key[e];
    if (best < minw[r]) ORIENT_MIN_U64(&minw[r], best);               // (the plain read may be old: then the min is merely redundant)
}
// (a2) among those of that weight, the least (lo, hi)
GSR_HD void orient_min_edge_vertex(int64_t v, const uint32_t* par, const int32_t* off, const int32_t* adj, const uint64_t* key, const uint64_t* minw,
                                   uint64_t* minlohi) {
    const uint32_t r = par[v] & ORIENT_PARENT;
    const uint64_t w = minw[r];
    if (w == ORIENT_NONE) return;
    uint64_t best = ORIENT_NONE;
    for (int32_t e = off[v]; e < off[v + 1]; ++e) {
        const uint32_t j = (uint32_t)adj[e];
        if (key[e] != w || (par[j] & ORIENT_PARENT) == r) continue;
        const uint64_t lohi = (uint32_t)v < j ? ((uint64_t)(uint32_t)v << 32 | j) : ((uint64_t)j << 32 | (uint32_t)v);
        if (lohi < best) best = lohi;
    }
    if (best < minlohi[r]) ORIENT_MIN_U64(&minlohi[r], best);
}
// (b) out[v] = in[v], except that a root with a chosen edge {x in it, y outside} hooks to the root of y with the parity
// flip[x] ^ flip[y] ^ (dot < 0).  Two roots that chose the same edge: the lower index stays.  Reads `in` only, so no lane sees
// another's hook.  Returns whether v hooked.
GSR_HD bool orient_hook_vertex(int64_t v, const uint32_t* in, uint32_t* out, const double* nrm, const uint64_t* minw, const uint64_t* minlohi) {
    const uint32_t word = in[v];
    out[v] = word;
    if ((word & ORIENT_PARENT) != (uint32_t)v || minw[v] == ORIENT_NONE || minlohi[v] == ORIENT_NONE) return false;
    const uint32_t lo = (uint32_t)(minlohi[v] >> 32), hi = (uint32_t)minlohi[v];
    const bool lo_in = (in[lo] & ORIENT_PARENT) == (uint32_t)v;
    const uint32_t x = lo_in ? lo : hi, y = lo_in ? hi : lo;
    const uint32_t ry = in[y] & ORIENT_PARENT;
    if (ry == (uint32_t)v) return false;                              // (cannot happen: the edge leaves the component)
    if (minw[ry] == minw[v] && minlohi[ry] == minlohi[v] && (uint32_t)v < ry) return false;
    const uint32_t neg = orient_dot(nrm, lo, hi) < 0.0 ? 1u : 0u;
    out[v] = ry | (((in[x] >> 31) ^ (in[y] >> 31) ^ neg) << 31);
    return true;
}
// (c) a parent walk of at most ORIENT_JUMPS hops, parities composed by XOR.  In place: whatever mixture of old and new words the
// walk reads, each is (an ancestor, the parity relative to it), so the word written is one too.
GSR_HD void orient_jump_vertex(int64_t v, uint32_t* par) {
    const uint32_t word = par[v];
    uint32_t p = word & ORIENT_PARENT, f = word >> 31;
    for (int hop = 0; hop < ORIENT_JUMPS; ++hop) {
        const uint32_t up = par[p];
        if ((up & ORIENT_PARENT) == p) break;
        p = up & ORIENT_PARENT;
        f ^= up >> 31;
    }
    const uint32_t now = p | (f << 31);
    if (now != word) par[v] = now;
}
// after the walks of a round: does v point at a root?  (a cycle from a hooking bug ends here, as an error code)
GSR_HD bool orient_is_flat(int64_t v, const uint32_t* par) {
    const uint32_t p = par[v] & ORIENT_PARENT;
    return (par[p] & ORIENT_PARENT) == p;
}

// ---- after the rounds ----------------------------------------------------------------------------------------------------------
// the vote of v: +1 toward the reference, -1 away, 0 none.  `lowest` is the lowest vertex of the component (its label): the
// orientation so far is relative to it.
GSR_HD int orient_vote_vertex(int64_t v, const uint32_t* par, const int32_t* label, const uint8_t* live, const float* xyz, const double* nrm, double cx,
                              double cy, double cz) {
    if (!live[v]) return 0;
    const double px = (double)xyz[v * 3], py = (double)xyz[v * 3 + 1], pz = (double)xyz[v * 3 + 2];
    if (!orient_finite3(px, py, pz)) return 0;
    const uint32_t flip = (par[v] >> 31) ^ (par[label[par[v] & ORIENT_PARENT]] >> 31);
    const double s = flip ? -1.0 : 1.0;                               // an exact negation of every product and sum
    const double t = (cx - px) * (s * nrm[v * 3]) + (cy - py) * (s * nrm[v * 3 + 1]) + (cz - pz) * (s * nrm[v * 3 + 2]);
    return t > 0.0 ? 1 : (t < 0.0 ? -1 : 0);
}
// the last step: negate the normal where the parity and the component's vote say so, write the label; returns ORIENT_IS_* bits
GSR_HD int orient_flip_vertex(int64_t v, const uint32_t* par, const int32_t* label, const uint8_t* live, const int32_t* toward, const int32_t* away,
                              bool vote, double* nrm, int32_t* component) {
    const uint32_t r = par[v] & ORIENT_PARENT;
    const int32_t lowest = label[r];
    if (component) component[v] = lowest;
    int what = r == (uint32_t)v ? ORIENT_IS_ROOT : 0;
    if (!live[v]) return what | ORIENT_IS_NOT_LIVE;
    uint32_t flip = (par[v] >> 31) ^ (par[lowest] >> 31);
    if (vote && away[r] > toward[r]) flip ^= 1u;
    if (flip) {
        nrm[v * 3] = -nrm[v * 3]; nrm[v * 3 + 1] = -nrm[v * 3 + 1]; nrm[v * 3 + 2] = -nrm[v * 3 + 2];
        what |= ORIENT_IS_FLIPPED;
    }
    return what;
}

// launches of the walk kernel after a round's hooks: the deepest chain has n - 1 links
inline int orient_jump_launches(int64_t n) {
    int launches = 1;
    for (int64_t reach = ORIENT_JUMPS; reach < n; reach *= ORIENT_JUMPS) ++launches;
    return launches + 1;
}

// the host's argument check of gsr_orient_normals_graph: NULL, or why the call is invalid
inline const char* orient_check_args(const float* xyz, const double* normals, int64_t n, const int32_t* nbr, int32_t stride, const int32_t* count,
                                     const double* reference) {
    if (n < 0) return "n < 0";
    if (n >= ((int64_t)1 << 31)) return "n must be below 2^31";
    if (stride < 1) return "stride must be >= 1";
    if (n * (int64_t)stride >= ((int64_t)1 << 30)) return "n * stride must be below 2^30";
    if (reference && !orient_finite3(reference[0], reference[1], reference[2])) return "the reference point is not finite";
    if (n > 0 && (!normals || !nbr || !count)) return "normals, nbr and count are required";
    if (n > 0 && reference && !xyz) return "xyz is required with a reference point";
    return nullptr;
}

}  // namespace gsr
