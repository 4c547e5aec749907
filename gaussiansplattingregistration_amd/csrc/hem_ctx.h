// hem_ctx.h -- the host side of a HEM context: everything a level needs before it runs.  The levels (Level), the context (gsr_hem_ctx), the
// glibc rand() jump tables and the flag draws, the read-backs (read_back, read_back_level), the scan and sort configurations and their
// wrappers, the level prologue, the phase-timing and checkpoint macros.  Included once by hem.hip, behind its kernels, which this code launches.
#pragma once

namespace gsr {

struct Level {
    int64_t n = 0;
    int F = 0;
    DevBuf xyz, color, cov6, opacity, weight, sh, is_parent;
    int32_t reserve(int64_t m, int f) {
        const size_t mm = (size_t)(m > 0 ? m : 1);
        GSR_TRY(xyz.reserve(mm * 3 * 4)); GSR_TRY(color.reserve(mm * 3 * 4)); GSR_TRY(cov6.reserve(mm * 6 * 4));
        GSR_TRY(opacity.reserve(mm * 4)); GSR_TRY(weight.reserve(mm * 4));
        GSR_TRY(sh.reserve(mm * (size_t)(f > 0 ? f : 1) * 4)); GSR_TRY(is_parent.reserve(mm));
        return GSR_OK;
    }
    void swap(Level& o) {
        std::swap(n, o.n); std::swap(F, o.F);
        xyz.swap(o.xyz); color.swap(o.color); cov6.swap(o.cov6); opacity.swap(o.opacity);
        weight.swap(o.weight); sh.swap(o.sh); is_parent.swap(o.is_parent);
    }
};

}  // namespace gsr

struct gsr_hem_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Stream aux;                     // second stream: the queue of heavy work items runs beside the light parents
    Event ev_fork, ev_join;
    Event ev_pre;                   // the parents' output ranks (flags in input order + their scan), computed beside the grid phase
    Stream aux2;                    // third stream: the SH rows are gathered into cell order (an HBM stream only the M-step needs)
    Event ev_sh_fork, ev_sh_join;   // beside the selection (VALU / latency bound)
    Event ev_halo;                  // partitioned level: the ghosts' SH rows have arrived (their exchange runs on aux2 beside the grid phase and the selection)
    Event evp[4];                   // brackets of the two halo exchanges (records on the main stream, SH rows on aux2)
    float part_ms[4] = {0, 0, 0, 0};                            // their durations (gsr_hem_get_part_ms)
    DevBuf sh_send;
    float rho = 3.0f, delta = 3.0f, kappa = 2.5f, tau = 1.0f;
    int rng_mode = GSR_RNG_GLIBC;
    uint32_t rng_seed = 1;
    uint64_t rng_pos = 0;           // hem::rand() values consumed so far
    unsigned rng_base[31];          // y_{-31..-1} of the seeded glibc stream
    bool rng_ready = false;
    Level cur, nxt, tmp;
    // level 0 borrowed from the caller (gsr_hem_set_level0, on_device = 2): `spare` keeps cur's own five big buffers meanwhile
    bool cur_borrowed = false;
    DevBuf spare[5];
    // gsr_hem_set_output: the next level is written straight into caller-owned arrays, which then ARE the current level (borrowed)
    void* out_ptr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t out_rows = 0;
    bool out_pending = false;
    DevBuf spare_out[5];            // nxt's own big arrays, parked while the caller's stand in for them
    bool have_level = false;
    // workspace
    DevBuf hist, iflag, irank, ipos, rng_blocks, bhist, bstart, bcursor;
    bool split_heavy = true;        // heavy parents are cut into work items of SEL_PART candidates (GSR_HEM_SPLIT=0: one wave per parent)
    bool sum_bucket = true;         // per-child sums by bucket partition + LDS fixed point (GSR_HEM_SUMLW=sort for the radix sort)
    // spatially partitioned levels (gsr_hem_set_comm + gsr_hem_set_level0_part): this rank owns cur.n components of a level of
    // n_global; gid = their global indices (ascending)
    gsr_comm* comm = nullptr;
    int64_t n_global = 0;
    DevBuf gid, gid_next, rec_loc, gid_loc, ghost_sh, ghost_src, perm, pown, ppos_own, inv, gmax, gacc, cmask, dflag, dpos, sent_idx, rows_send, rows_recv,
        xsend, xrecv, gbits, wcnt, wpre, grank, allflags, pcounts, pmatrix;
    int64_t part_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // ghosts, rows sent, bytes received in the halo exchange, bytes of the other exchanges, ...
    int partition_stage = 0;        // GSR_HEM_PARTITION_STAGE=6144 / 4096: force a smaller stage than the bucket count asks for (tests)
    bool partition_staged = true;   // k_partition<STAGE > 0>: pairs staged by bucket in LDS, read once (GSR_HEM_PARTITION=walk: the two-walk form)
    bool partition_fixed = true;    // bucket regions of fixed capacity filled straight from the segments (GSR_HEM_PARTITION=exact: histogram + scan)
    bool partition_overflowed = false;      // a region overflowed once: this context uses the exact partition from then on
    double partition_factor = 0.0;  // GSR_HEM_PARTITION_FACTOR: region capacity in multiples of the mean (test knob: < 1 forces the overflow path)
    PinnedBlock host_rb;            // unsigned long long[64], the device writes read-backs into it: [0..14] k_collect, [15] sequence number, [16..31] k_level_collect
    unsigned long long rb_seq = 0;
    bool rb_poll = true;            // the host polls the sequence word (GSR_HEM_RB_POLL=0: hipStreamSynchronize)
    DevBuf rec, bbox, bbox_part, gparams, keys, idx, skeys, order, cellStart, A, geo, shs, Rs, pflag, ppos, plist;
    DevBuf pcap, coff, sp_child, sp_wl, porder, pkeys, pkeys2, pidx, mhdr, prec, rowlist;
    int sh_policy = 2;              // the cell-sorted, padded copy of the SH block (k_gather_sh) the M-step reads its children's rows from: 2 (default) = decided
                                    // per level ON THE DEVICE -- made iff the level has at least sh_direct_pairs accepted pairs per component, else the rows are
                                    // read from the level's own array; GSR_HEM_SH_DIRECT=0: always made (rounds 1-4), =1: never; GSR_HEM_SH_DIRECT_PAIRS=x: the
                                    // threshold.  Measured at 5 M (profiles/r05e_ab_sh_direct.txt), level time copy / no copy: isotropic (22 pairs per component)
                                    // 8.54 / 8.50 ms from own buffers but 8.63 / 8.78 in the bench's zero-copy cascade; clustered (7) 6.98 / 6.70; surfels (2) 6.55 / 6.25
    float sh_direct_pairs = 8.0f;
    bool use_rowlist = true;        // GSR_HEM_ROWLIST=0: k_select computes every row span itself instead of taking the non-empty ones from k_spans
    size_t rowlist_max = (size_t)4096 << 20;   // GSR_HEM_ROWLIST_MAX_MB: the row lists are 256 bytes per parent (0.43 GB at the 1.67 M parents of a 5 M level,
                                    // 3.4 GB at 40 M splats), kept by the context; a level whose lists would be larger runs without them
    int timing = 1;                 // gsr_hem_set_timing / GSR_HEM_TIMING: 0 no events, 1 level + k_select + k_mstep, 2 every phase (see GSR_TIME)
    int select_np = 0;              // GSR_HEM_SELECT_NP=1|2|4: light parents per selection wave (the rings are kept across them, see SEL_NP); 0 = by level size
    bool mstep_split = true;        // GSR_HEM_MSTEP_SPLIT=0: a parent of more than MSTEP_SEG pairs keeps ONE wave for all its segments (the schedule of rounds 1-3)
    DevBuf mh_list, mh_items, mh_scratch;
    Event ev_mfork, ev_mjoin;       // the heavy parents' segments run on the second stream beside k_mstep
    bool mstep_small = true;        // GSR_HEM_MSTEP_SMALL=0: no four-at-a-time path for the parents of <= 16 pairs (test knob: nothing may change)
    bool use_ell = true;            // GSR_HEM_ELL=0: no ellipsoid row clipping (test knob: the pair set must not change)
    int shard_rank = 0, shard_world = 1;      // work-sharded level: parents split over ranks, data replicated
    gsr_allreduce_dev_fn shard_allreduce = nullptr;
    gsr_allgather_dev_fn shard_allgather = nullptr;
    void* shard_user = nullptr;
    DevBuf shard_send, shard_recv;
    bool sparse_path = false;
    DevBuf hitem, hfirst, part_cnt, Ac, cellStartC, cellStartI;
    DevBuf pcnt, poff, pair_child, pair_wl, spair_child, spair_wl, cstart, sumLw, oflag, pflag_in, oflag_in, prank_in, orank_in;
    DevBuf keep, kpos, scratch, draws, counters, rocprim_tmp, rocprim_tmp2, sh_tail, holes, erase_halo;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t stats_ex[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float phase_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Event ev[8];
    Event evk[4];                   // brackets of k_select<COUNT> and k_select<FILL>
    Event evm[6];                   // brackets of k_mstep, k_partition, k_bucket_sum
    float kernel_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // The PROLOGUE of a level -- packed records, bounding box, axis histograms, grid geometry, the counts of parents and irregular
    // components: everything the host needs before it can size and launch the level -- is computed when the level's INPUT comes into
    // being (gsr_hem_set_level0, the end of the level before), and its answer rides in that moment's round trip.  pro.valid: `rec`,
    // `gparams` and the counter block pro.cblock hold it for the current level of pro.n components.
    struct Prologue { bool valid = false; GridParams gp; int P = 0, n_irr = 0, cblock = 0; int64_t n = 0; float ms = 0.0f; } pro;
    Event ev_pro[2];                // brackets of a prologue: its time counts for the level that consumes it (pro.ms)
    int cblock = 0;                 // which of the two counter blocks the running level uses (the next level's prologue clears the other)
    DevBuf lvl;                     // long long[8]: device-resident counts of an asynchronous level (k_level_tail); [2] = work-item size (k_heavy_items)
    bool async_ok = true;           // GSR_HEM_ASYNC=0: every level sizes its buffers from counts read back on the way (five round trips, the rounds 1-4 schedule)
    bool last_level = false;        // gsr_hem_run_levels: the level being run is the last of its hierarchy -- no prologue of a next level behind it
    Stream side;                    // gsr_hem_run_levels: the levels' normals beside the next level (created on first use, with its events)
    Event ev_side, ev_side_fork;
    int round_trips = 0;            // host round trips of the last gsr_hem_run_level (statistic: gsr_hem_get_stats_ex [6])
    int was_async = 0;              // the last level ran without a round trip between its first and its last kernel ([7])
    float cell_target = 16.0f;      // components per grid cell (GSR_HEM_CELL_TARGET; the result does not depend on it).  Swept at 5 M after the parents left
                                    // the candidate stream: 5 -> 13.15 ms per level, 8 -> 12.87, 12 -> 12.70, 16 -> 12.61, 24 -> 12.60, 32 -> 12.68 (fewer, longer rows)
    int max_cells = 1 << 24;
    ~gsr_hem_ctx();
};

namespace {

// x^(2^b) mod (x^31 - x^28 - 1) over Z/2^32, b = 0..47 (host, once)
void rng_polymul(const unsigned* a, const unsigned* b, unsigned* out) {
    unsigned prod[61];
    for (int d = 0; d < 61; ++d) prod[d] = 0;
    for (int i = 0; i < 31; ++i) for (int j = 0; j < 31; ++j) prod[i + j] += a[i] * b[j];
    for (int d = 60; d >= 31; --d) { const unsigned c = prod[d]; prod[d - 3] += c; prod[d - 31] += c; }
    for (int d = 0; d < 31; ++d) out[d] = prod[d];
}
const unsigned* rng_xpow_table() {
    struct Table {                       // function-local static: initialised once, thread-safely (C++11)
        unsigned tab[48 * 31];
        Table() {
            for (int j = 0; j < 31; ++j) tab[j] = j == 1 ? 1u : 0u;             // x^1
            for (int b = 1; b < 48; ++b) rng_polymul(tab + (b - 1) * 31, tab + (b - 1) * 31, tab + b * 31);
        }
    };
    static const Table t;
    return t.tab;
}

// draw n parent flags in order into dst (consumes n hem::rand() values)
// (n_dev: n is only a bound -- the launch is sized for it -- and the real count lies on the device; the caller then sets the stream
// position itself once it knows the count)
int32_t draw_flags_raw(gsr_hem_ctx* c, int64_t n, uint8_t* dst, hipStream_t on = nullptr, const long long* n_dev = nullptr) {
    const hipStream_t fst = on ? on : c->stream;
    const float prob = 1.0f / c->rho;
    if (n == 0) return GSR_OK;
    if (c->rng_mode == GSR_RNG_HASH) {
        hipLaunchKernelGGL(k_flags_hash, dim3(stride_grid(n)), dim3(256), 0, fst, n, c->rng_seed,
                           (unsigned long long)c->rng_pos, prob, dst, n_dev);
        c->rng_pos += (uint64_t)n;
        return GSR_OK;
    }
    if (!c->rng_ready) {                      // seed words and the jump table, once per context / reseed
        unsigned st[31];
        {   // srand(seed) fills 31 words (Schrage LCG); keep them BEFORE the 310 discarded outputs
            uint32_t s = c->rng_seed ? c->rng_seed : 1u;
            int32_t word = (int32_t)s;
            st[0] = (unsigned)word;
            for (int i = 1; i < 31; ++i) {
                int32_t hi = word / 127773, lo = word % 127773;
                word = 16807 * lo - 2836 * hi;
                if (word < 0) word += 2147483647;
                st[i] = (unsigned)word;
            }
        }
        for (int j = 0; j < 31; ++j) c->rng_base[j] = st[(j + 3) % 31];        // y_{-31+j} = x_{(j+3) mod 31}
        // device tables: x^(2^b), the per-thread jumps x^(8 * RNG_ELEMS * t), and the sequence continued from the seed state
        std::vector<unsigned> tab(RNG_TAB_WORDS, 0u);
        memcpy(tab.data() + RNG_TAB_XPOW, rng_xpow_table(), 48 * 31 * 4);
        {
            unsigned step[31], cur[31], nxt[31];
            for (int j = 0; j < 31; ++j) { step[j] = j == 0 ? 1u : 0u; cur[j] = step[j]; }
            for (int b = 0; b < 48; ++b)
                if (((unsigned long long)(8 * RNG_ELEMS) >> b) & 1ull) { rng_polymul(step, rng_xpow_table() + b * 31, nxt); memcpy(step, nxt, sizeof(step)); }
            for (int t = 0; t < RNG_THREADS; ++t) {
                for (int j = 0; j < 31; ++j) tab[RNG_TAB_T + j * 64 + t] = cur[j];
                rng_polymul(cur, step, nxt);
                memcpy(cur, nxt, sizeof(cur));
            }
        }
        for (int m = 0; m < 91; ++m)
            tab[RNG_TAB_YBASE + m] = m < 31 ? c->rng_base[m] : tab[RNG_TAB_YBASE + m - 3] + tab[RNG_TAB_YBASE + m - 31];
        GSR_TRY(c->draws.reserve(RNG_TAB_WORDS * 4));
        GSR_HIP(hipMemcpy(c->draws.p, tab.data(), RNG_TAB_WORDS * 4, hipMemcpyHostToDevice));
        c->rng_ready = true;
    }
    const int64_t nblocks = (n + RNG_BLOCK_ELEMS - 1) / RNG_BLOCK_ELEMS;
    GSR_TRY(c->rng_blocks.reserve((size_t)nblocks * 64 * 4));
    hipLaunchKernelGGL(k_rng_block_state, dim3((unsigned)nblocks), dim3(64), 0, fst, (unsigned long long)c->rng_pos,
                       c->draws.as<unsigned>(), c->rng_blocks.as<unsigned>(), n_dev);
    hipLaunchKernelGGL(k_flags_glibc, dim3((unsigned)nblocks), dim3(RNG_THREADS), 0, fst, n, prob, c->draws.as<unsigned>(),
                       c->rng_blocks.as<unsigned>(), dst, n_dev);
    c->rng_pos += (uint64_t)n;
    return GSR_OK;
}
int32_t draw_flags(gsr_hem_ctx* c, Level& lv) { return draw_flags_raw(c, lv.n, lv.is_parent.as<uint8_t>()); }

// (the wait of a round trip: the kernel that carries sequence number `seq` has been enqueued on the context's stream)
int32_t wait_round_trip(gsr_hem_ctx* c, unsigned long long seq) {
    c->round_trips += 1;
    return wait_host_flag(c->stream, c->host_rb.as<unsigned long long>() + 15, seq, c->rb_poll);
}
int32_t read_back(gsr_hem_ctx* c, const Collect& q, unsigned long long* out) {
    const unsigned long long seq = ++c->rb_seq;
    hipLaunchKernelGGL(k_collect, dim3(1), dim3(8), 0, c->stream, q, c->host_rb.as<unsigned long long>(), seq);
    GSR_HIP(hipGetLastError());
    GSR_TRY(wait_round_trip(c, seq));
    for (int i = 0; i < q.n; ++i) out[i] = __atomic_load_n(c->host_rb.as<unsigned long long>() + i, __ATOMIC_RELAXED);
    return GSR_OK;
}
// the level-wide answer (k_level_collect): LC_WORDS words
int32_t read_back_level(gsr_hem_ctx* c, const LevelCollect& q, unsigned long long* out) {
    const unsigned long long seq = ++c->rb_seq;
    hipLaunchKernelGGL(k_level_collect, dim3(1), dim3(64), 0, c->stream, q, c->host_rb.as<unsigned long long>(), seq);
    GSR_HIP(hipGetLastError());
    GSR_TRY(wait_round_trip(c, seq));
    for (int i = 0; i < LC_WORDS; ++i) out[i] = __atomic_load_n(c->host_rb.as<unsigned long long>() + 16 + i, __ATOMIC_RELAXED);
    return GSR_OK;
}

// (side = true: on the context's second stream, with its own temporary storage)
// rocPRIM's look-back scan with more items per thread on large inputs (its default for gfx950: 30 us per 5 M ints; 256 threads x 64 items:
// 19 us; int64 sums of 1.67 M counts 19.5 -> 12 us with 32 items: profiles/r05ak_scan_configs.txt) -- on small inputs the default's
// many small workgroups are the better shape
#ifndef GSR_SCAN_BIG_N
#define GSR_SCAN_BIG_N (1 << 20)
#endif
using scan_cfg_big = rocprim::scan_config<256, 64, rocprim::block_load_method::block_load_transpose, rocprim::block_store_method::block_store_transpose,
                                          rocprim::block_scan_algorithm::using_warp_scan>;
using scan_cfg64_big = rocprim::scan_config<256, 32, rocprim::block_load_method::block_load_transpose, rocprim::block_store_method::block_store_transpose,
                                            rocprim::block_scan_algorithm::using_warp_scan>;
template <typename T>
int32_t exclusive_scan(gsr_hem_ctx* c, const T* in, T* out, int64_t n, bool side = false) {
    const hipStream_t s = side ? c->aux : c->stream;
    DevBuf& tmp = side ? c->rocprim_tmp2 : c->rocprim_tmp;
    if (n >= GSR_SCAN_BIG_N) return scan_exclusive<scan_cfg_big>(tmp, s, in, out, (size_t)n);
    return scan_exclusive<rocprim::default_config>(tmp, s, in, out, (size_t)n);
}

// rocPRIM's Onesweep with its gfx950 kernel shapes but 10 bits per pass: the 19-bit cell keys of a 5 M level take two passes
// instead of three (grid phase 1.21 -> 1.15 ms; 11 bits: no further gain).  Up to 2^20 keys rocPRIM's merge sort runs as before.
#ifndef GSR_SORT_RADIX_BITS
#define GSR_SORT_RADIX_BITS 10
#endif
// GSR_SORT_MERGE_LIMIT: up to this many keys rocPRIM sorts by block sort + merge passes (~20 launches at 5 * 10^5 keys), beyond it by Onesweep
#ifndef GSR_SORT_MERGE_LIMIT
#define GSR_SORT_MERGE_LIMIT (256 * 1024)      // measured on the bench levels (profiles/archive/r04i): 1 M -> 256 k takes 0.05 ms off the 1.67 M level (its 556 k parents) and 0.04 off the 556 k level; 128 k, 32 k: the same
#endif
#ifndef GSR_SORT_BS
#define GSR_SORT_BS 1024
#endif
#ifndef GSR_SORT_IPT
#define GSR_SORT_IPT 12        // keys per thread of the Onesweep kernels (1 024 threads): 16 -> 12 takes 44 us off a 5 M level's two sorts (230 -> 186 us;
                               // 10 the same, 8: 198, 4: 243; 512- and 256-thread workgroups 260 ... 600 us), profiles/r05ah_onesweep_configs.txt
#endif
// (the sorts of up to GSR_SORT_MERGE_LIMIT keys: block sort of 1 024 x 8 keys, then merge passes -- 20 us less per 200 k-splat level than rocPRIM's
// default shape, equal at 50 k and 556 k: profiles/r05am_merge_sort_configs.txt)
#ifndef GSR_MERGE_SORT_BS
#define GSR_MERGE_SORT_BS 1024
#define GSR_MERGE_SORT_IPT 8
#define GSR_MERGE_MP_BS 128
#define GSR_MERGE_MP_IPT 4
#endif
using merge_cfg = rocprim::merge_sort_config<512, GSR_MERGE_SORT_BS, GSR_MERGE_SORT_IPT, 128, GSR_MERGE_MP_BS, GSR_MERGE_MP_IPT>;
using sort_cfg = rocprim::radix_sort_config<rocprim::default_config, merge_cfg,
                                            rocprim::radix_sort_onesweep_config<rocprim::kernel_config<GSR_SORT_BS, GSR_SORT_IPT>, rocprim::kernel_config<GSR_SORT_BS, GSR_SORT_IPT>, GSR_SORT_RADIX_BITS,
                                                                                rocprim::block_radix_rank_algorithm::match>,
                                            GSR_SORT_MERGE_LIMIT>;
// the ordering sort (parents by work class + block of space, ORDER_KEY_BITS + 2 bits): when its key fits ONE Onesweep pass the merge sort's
// block sort + log2(n / 8192) merge passes lose from a few ten thousand keys on
#ifndef GSR_ORDER_MERGE_LIMIT
#define GSR_ORDER_MERGE_LIMIT 16384
#endif
using order_cfg = rocprim::radix_sort_config<rocprim::default_config, merge_cfg,
                                             rocprim::radix_sort_onesweep_config<rocprim::kernel_config<GSR_SORT_BS, GSR_SORT_IPT>, rocprim::kernel_config<GSR_SORT_BS, GSR_SORT_IPT>, GSR_SORT_RADIX_BITS,
                                                                                 rocprim::block_radix_rank_algorithm::match>,
                                             GSR_ORDER_MERGE_LIMIT>;
template <typename V, typename CFG = sort_cfg>
int32_t sort_pairs(gsr_hem_ctx* c, const unsigned* kin, unsigned* kout, const V* vin, V* vout, int64_t n, int end_bit) {
    return sort_pairs_by_key<CFG>(c->rocprim_tmp, c->stream, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)end_bit);
}

// launch_partition's mode, out of the GSR_HEM_PARTITION / GSR_HEM_PARTITION_STAGE knobs
static inline int partition_mode(const gsr_hem_ctx* c) { return c->partition_staged ? (c->partition_stage ? c->partition_stage : 1) : 0; }

int bits_for(int64_t n) {
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) < n) ++b;
    return b;
}

// cur.{xyz,color,cov6,opacity,sh} <-> the caller's arrays (borrowed) / the context's own buffers (spare)
inline DevBuf* level_big(Level& L, int i) { DevBuf* b[5] = {&L.xyz, &L.color, &L.cov6, &L.opacity, &L.sh}; return b[i]; }
void unborrow_level0(gsr_hem_ctx* c) {
    if (!c->cur_borrowed) return;
    for (int i = 0; i < 5; ++i) {
        DevBuf* b = level_big(c->cur, i);
        b->release();                               // the caller's memory: let go, never freed
        b->swap(c->spare[i]);
    }
    c->cur_borrowed = false;
}
}  // namespace
// the members free themselves (on the context's device); a borrowed level 0 goes back to the caller first, cur gets its own buffers again
gsr_hem_ctx::~gsr_hem_ctx() {
    (void)hipSetDevice(device);
    unborrow_level0(this);
}
namespace {

// The prologue of the level whose input is L (gsr_hem_ctx::Prologue): k_prep (the packed records, box partials, the counts of parents
// and irregular components), their fold (which also clears the level's counter block and the histograms), the axis histograms, the grid
// geometry.  n_dev != NULL: the level's size lies on the device (the level before has not reported yet) and n is a bound for the grids.
int32_t enqueue_prologue(gsr_hem_ctx* c, Level& L, int64_t n, const long long* n_dev, int cblock) {
    hipStream_t st = c->stream;
    const dim3 blk(256), grd(stride_grid(n));
    GSR_TRY(c->rec.reserve((size_t)n * 64)); GSR_TRY(c->bbox.reserve(64));
    GSR_TRY(c->gparams.reserve(sizeof(GridParams))); GSR_TRY(c->counters.reserve(128));
    GSR_TRY(c->bbox_part.reserve((size_t)grd.x * 8 * 4)); GSR_TRY(c->hist.reserve(3 * HIST_BINS * 4));
    GSR_TRY(c->bcursor.reserve(((size_t)SUM_MAX_BUCKETS + 1) * 8));
    if (c->timing >= 1) GSR_HIP(hipEventRecord(c->ev_pro[0], st));
    hipLaunchKernelGGL(k_prep, grd, blk, 0, st, n, L.xyz.as<float>(), L.color.as<float>(), L.cov6.as<float>(), L.opacity.as<float>(),
                       L.weight.as<float>(), L.is_parent.as<uint8_t>(), c->rec.as<float4>(), c->bbox_part.as<unsigned>(), n_dev);
    hipLaunchKernelGGL(k_bbox_reduce, dim3(1), dim3(256), 0, st, (int)grd.x, c->bbox_part.as<unsigned>(), c->bbox.as<unsigned>(),
                       c->counters.as<unsigned>() + 16 * cblock, 16, c->hist.as<unsigned>(), 3 * HIST_BINS, c->bcursor.as<unsigned>(), SUM_MAX_BUCKETS + 1);
    hipLaunchKernelGGL(k_hist, dim3(stride_grid(n) > 512 ? 512 : stride_grid(n)), blk, 0, st, n, L.xyz.as<float>(), c->bbox.as<unsigned>(), c->hist.as<unsigned>(), n_dev);
    hipLaunchKernelGGL(k_grid_params, dim3(1), dim3(64), 0, st, c->bbox.as<unsigned>(), c->hist.as<unsigned>(), n, c->cell_target,
                       c->max_cells, c->gparams.as<GridParams>(), n_dev);
    if (c->timing >= 1) GSR_HIP(hipEventRecord(c->ev_pro[1], st));
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}
// ... and its answer, out of the words of k_level_collect
void take_prologue(gsr_hem_ctx* c, const unsigned long long* w, int64_t n, int cblock) {
    static_assert(sizeof(GridParams) == 40 && LC_NEXT_GP + 5 == LC_WORDS, "GridParams travels as five 8-byte words");
    memcpy(&c->pro.gp, w + LC_NEXT_GP, sizeof(GridParams));
    c->pro.P = (int)(unsigned)w[LC_NEXT_P]; c->pro.n_irr = (int)(unsigned)w[LC_NEXT_IRR];
    c->pro.n = n; c->pro.cblock = cblock; c->pro.valid = true;
    c->pro.ms = 0.0f;
    if (c->timing >= 1) (void)hipEventElapsedTime(&c->pro.ms, c->ev_pro[0], c->ev_pro[1]);      // (both have completed: the round trip came behind them)
}
// The current level's prologue, now, with its own round trip (gsr_hem_set_level0, gsr_hem_set_state, a level whose prologue is not there).
// Partitioned / work-sharded levels compute theirs inside the level (their box and histograms are all-reduced over the ranks).
int32_t prologue_now(gsr_hem_ctx* c) {
    c->pro.valid = false;
    if (c->cur.n <= 0 || c->comm != nullptr || c->shard_world > 1) return GSR_OK;
    const int cb = c->cblock ^ 1;
    GSR_TRY(enqueue_prologue(c, c->cur, c->cur.n, nullptr, cb));
    LevelCollect q;
    memset(&q, 0, sizeof(q));
    q.cnt = c->counters.as<int>() + 16 * cb; q.gp = c->gparams.as<GridParams>(); q.bbox = c->bbox.as<unsigned>();
    unsigned long long w[LC_WORDS];
    GSR_TRY(read_back_level(c, q, w));
    take_prologue(c, w, c->cur.n, cb);
    return GSR_OK;
}
}  // namespace

// GSR_HEM_DEBUG_SYNC=1: synchronise and report after every stage of a level (localises a device fault)
// Always: a failed LAUNCH of the stage just enqueued (bad configuration, too much LDS) is reported with the stage's name.
// The events between the phases (gsr_hem_get_phase_ms / _kernel_ms).  An event record between two kernels is a barrier packet of its
// own, 22 per level: 0.1 ms of a 5 M level, 6 % of a 556 k one.  gsr_hem_set_timing: 0 = none, 1 (default) = the level and the two
// dominant kernels (GSR_TIME1), 2 = every phase.
#define GSR_TIME(ev, stream) do { if (c->timing >= 2) GSR_HIP(hipEventRecord(ev, stream)); } while (0)
#define GSR_TIME1(ev, stream) do { if (c->timing >= 1) GSR_HIP(hipEventRecord(ev, stream)); } while (0)
#define GSR_CHECKPOINT(label)                                                                       \
    do {                                                                                            \
        {                                                                                           \
            const hipError_t _l = hipGetLastError();                                                \
            if (_l != hipSuccess) return fail(GSR_E_HIP, "%s: launch failed: %s", label, hipGetErrorString(_l)); \
        }                                                                                           \
        if (dbg_sync) {                                                                             \
            hipError_t _e = hipStreamSynchronize(st);                                               \
            fprintf(stderr, "[gsr_hem] %s: %s\n", label, hipGetErrorString(_e));                    \
            fflush(stderr);                                                                         \
            if (_e != hipSuccess) return fail(GSR_E_HIP, "%s: %s", label, hipGetErrorString(_e));   \
        }                                                                                           \
    } while (0)
