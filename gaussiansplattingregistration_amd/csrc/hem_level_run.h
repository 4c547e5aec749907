// hem_level_run.h -- the driver of one HEM level (LevelRun: its status code, its stages).  Included once by hem.hip, behind hem_part_level.h.
#pragma once

namespace {

// internal status of LevelRun::run: the buffers an asynchronous level ran on were too small (or one of its other assumptions did not hold);
// nothing of the level's input has been touched -- gsr_hem_run_level runs it again the synchronous way, which sizes everything exactly
constexpr int32_t GSR_RETRY_SYNC = -1000;

// One level (gsr_hem_run_level), stage by stage.  Two schedules through the same stages:
//  * SYNCHRONOUS (rounds 1-4; still what a partitioned / work-sharded level, a fresh context and every fallback path run): the host sizes each
//    stage's buffers from counts it reads back on the way -- candidates, pairs, orphans, surviving rows: four round trips inside the level;
//  * ASYNCHRONOUS (`spec`, the default once the context's buffers exist): NO round trip between the level's first and its last kernel.
//    What the host knows when it starts is the level's prologue (grid, parents, irregular components: computed when the level's input came
//    into being); everything else stays on the device -- the heavy threshold and the work-item size come from the capacities' scan
//    (k_heavy_keys, k_heavy_items), the pair buffers are the ones the context has and every segment write is clamped to them (k_select),
//    the bucket regions take their capacity from the buffers, the new level's size is k_level_tail's, launches are sized for bounds and
//    their surplus blocks leave on the device count -- and ONE answer comes back behind the last kernel (k_level_collect) together with
//    the NEXT level's prologue.  A raised abort / overflow flag there means the level is run again synchronously (GSR_RETRY_SYNC);
//    its input was never written.
// The reference's level is one function without such a boundary (src/cpp_ext/src/mixture.cpp:25-35, 66-285).
struct LevelRun {
    gsr_hem_ctx* c;
    hipStream_t st;
    Level& L;
    Level& O;
    const bool dbg_sync, part, sharded;
    bool spec = false;
    const int sh_policy;                    // the cell-sorted copy of the SH block: 0 always made, 1 never (rows read from the level's own array), 2 decided on
                                            // the device by the level's pairs per component (k_gather_sh); a partitioned level: 0 (its ghosts' rows lie elsewhere)
    const int64_t n_own;
    int64_t n;
    const int F, RSH;
    PartLevel pl;
    const dim3 blk{256};
    dim3 grd;
    GridParams gp;
    int P_all = 0, P = 0, n_irr = 0;
    int* cnt = nullptr;                     // this level's counter block: [0] [1] heavy parents / segments of the M-step, [2] abort, [3] erased rows,
                                            // [8] heavy parents of the selection, [10] [11] their queue, [12] bucket overflow, [13] item table overflow, [15] max pairs
    long long* lvl = nullptr;               // device: [0] rows of the new level before the erase, [1] orphans, [2] (as unsigned) work-item size
    const float4* rec_src = nullptr;
    bool ranks_forked = false, sh_pending = false, sh_launched = false, flags_forked = false;
    // selection
    SelectArgs sa;
    size_t Pm = 1;
    int own_lo = 0, own_hi = 0;
    int64_t M = 0;
    unsigned long long cand = 0, cap_pairs = 0;
    // per-child sums
    const int64_t* seg = nullptr;
    const unsigned* pc = nullptr;
    const float* pw = nullptr;
    int bshift = 0, nbuckets = 0;
    int* overflow_flag = nullptr;
    bool fixed_tried = false;
    // output
    int64_t n_orph = 0, n_pre = 0, out_cap = 0;
    bool out_active = false;                // the new level is being written into the caller's arrays (gsr_hem_set_output)
    uint64_t rng_pos0 = 0;
    int64_t dropped = 0, P_glob = 0, O_glob = 0, n_pre_glob = 0, n_glob_next = 0;
    float pro_ms = 0.0f;                    // the time of this level's prologue, which ran when its input came into being

    LevelRun(gsr_hem_ctx* ctx, bool allow_async)
        : c(ctx), st(ctx->stream), L(ctx->cur), O(ctx->nxt), dbg_sync(getenv("GSR_HEM_DEBUG_SYNC") != nullptr), part(ctx->comm != nullptr),
          sharded(ctx->shard_world > 1 && ctx->shard_allreduce != nullptr), sh_policy(ctx->comm == nullptr ? ctx->sh_policy : 0), n_own(ctx->cur.n), n(ctx->cur.n), F(ctx->cur.F), RSH((ctx->cur.F + 3) & ~3) {
        spec = allow_async;
        pl.c = c; pl.st = st; pl.n_own = n_own;
        memset(&sa, 0, sizeof(sa));
    }
    ~LevelRun() {       // an error return hands nxt its own buffers back
        if (out_active) for (int i = 0; i < 5; ++i) { DevBuf* b = level_big(c->nxt, i); b->release(); b->swap(c->spare_out[i]); }
    }

    int32_t run(int64_t* n_out, int64_t* n_dropped);
    int32_t grid_phase();
    int32_t select_phase();
    int32_t sums_phase();
    int32_t sums_fixed();
    int32_t sums_exact();
    int32_t compact_pairs();
    int32_t output_ranks();
    int32_t open_output();
    int32_t mstep_phase();
    int32_t flags_and_validity();
    int32_t compact_erased(int64_t n_keep);
    int32_t erase_in_place(int64_t rows_bound, bool may_allocate, int64_t alloc_rows = 0);
    bool erase_on_device = false;           // the erase kernels were enqueued (an asynchronous level without the tails' buffer leaves the erase to the host)
    int32_t launch_gather_sh(bool fork);
    int32_t widen_scan(const unsigned* cnt_in, int64_t* off, int64_t count);
    int32_t total_of(const int64_t* off, const unsigned* cnt_in, int64_t count, int64_t* out);
};

struct WidenU32 { __device__ __host__ int64_t operator()(unsigned v) const { return (int64_t)v; } };
int32_t LevelRun::widen_scan(const unsigned* cnt_in, int64_t* off, int64_t count) {      // off = exclusive scan of cnt_in (int64)
    // (the counts are widened on the fly by the scan's input iterator: a separate transform pass was a launch and 12 bytes per count)
    auto in = rocprim::make_transform_iterator(cnt_in, WidenU32());
    size_t bytes = 0;
    if (count >= GSR_SCAN_BIG_N) {
        GSR_HIP(rocprim::exclusive_scan<scan_cfg64_big>(nullptr, bytes, in, off, (int64_t)0, (size_t)count, rocprim::plus<int64_t>(), st));
        GSR_TRY(c->rocprim_tmp.reserve(bytes));
        GSR_HIP(rocprim::exclusive_scan<scan_cfg64_big>(c->rocprim_tmp.p, bytes, in, off, (int64_t)0, (size_t)count, rocprim::plus<int64_t>(), st));
        return GSR_OK;
    }
    GSR_HIP(rocprim::exclusive_scan(nullptr, bytes, in, off, (int64_t)0, (size_t)count, rocprim::plus<int64_t>(), st));
    GSR_TRY(c->rocprim_tmp.reserve(bytes));
    GSR_HIP(rocprim::exclusive_scan(c->rocprim_tmp.p, bytes, in, off, (int64_t)0, (size_t)count, rocprim::plus<int64_t>(), st));
    return GSR_OK;
}
int32_t LevelRun::total_of(const int64_t* off, const unsigned* cnt_in, int64_t count, int64_t* out) {
    Collect q;
    q.n = 2;
    q.src[0] = off + (count - 1); q.bytes[0] = 8;
    q.src[1] = cnt_in + (count - 1); q.bytes[1] = 4;
    unsigned long long w[8];
    GSR_TRY(read_back(c, q, w));
    *out = (int64_t)w[0] + (int64_t)(unsigned)w[1];
    return GSR_OK;
}

// only the M-step reads the sorted SH rows: the gather (1.9 GB of HBM traffic at 5 M) can run on its own stream beside the
// selection, which is bound by VALU issue and load latency, and is joined in front of the M-step.  sh_overlap: 0 = in line
// here, 1 = forked here (beside the rest of the grid phase), 2 = forked just in front of k_select
int32_t LevelRun::launch_gather_sh(bool fork) {
    if (F <= 0) return GSR_OK;
    hipStream_t sst = st;
    if (fork) {
        GSR_HIP(hipEventRecord(c->ev_sh_fork, st)); GSR_HIP(hipStreamWaitEvent(c->aux2, c->ev_sh_fork, 0));
        sst = c->aux2;
    }
    const int shg = stride_grid(n * (RSH >> 2));
    if (part)
        hipLaunchKernelGGL(k_gather_sh2, dim3(shg), blk, 0, sst, n, n_own, F, RSH, c->order.as<unsigned>(), L.sh.as<float>(),
                           c->ghost_sh.as<float>(), c->shs.as<float>());
    else
        hipLaunchKernelGGL(k_gather_sh, dim3(shg), blk, 0, sst, n, F, RSH, c->order.as<unsigned>(), L.sh.as<float>(), c->shs.as<float>(),
                           P > 0 ? c->poff.as<int64_t>() : (const int64_t*)nullptr, c->pcnt.as<unsigned>(), P, sh_policy, c->sh_direct_pairs,
                           reinterpret_cast<int*>(lvl + 3));
    if (fork) { GSR_HIP(hipEventRecord(c->ev_sh_join, c->aux2)); sh_pending = true; }
    return GSR_OK;
}

// ---- 1. the level's prologue (det, packed records, bounding box, grid) if it is not there yet; sort by cell; the cell-sorted working set ----
int32_t LevelRun::grid_phase() {
    GSR_TRY(c->counters.reserve(128)); GSR_TRY(c->lvl.reserve(64));
    lvl = c->lvl.as<long long>();
    if (!part && !sharded) {
        // the prologue came with the level's input (gsr_hem_set_level0, the level before); if not -- a caller changed the flags, an error
        // path -- it is computed now, with a round trip of its own
        if (!(c->pro.valid && c->pro.n == n)) GSR_TRY(prologue_now(c));
        if (!c->pro.valid) return fail(GSR_E_INVALID, "gsr_hem_run_level: no prologue for the level");
        gp = c->pro.gp; P_all = c->pro.P; n_irr = c->pro.n_irr; c->cblock = c->pro.cblock; pro_ms = c->pro.ms;
        c->pro.valid = false;                   // consumed: `rec` and the counter block belong to this level now
        cnt = c->counters.as<int>() + 16 * c->cblock;
    } else {
        c->pro.valid = false;
        c->cblock ^= 1;
        cnt = c->counters.as<int>() + 16 * c->cblock;
        GSR_TRY(c->rec.reserve(n * 64)); GSR_TRY(c->bbox.reserve(64));
        GSR_TRY(c->gparams.reserve(sizeof(GridParams)));
        GSR_TRY(c->bbox_part.reserve((size_t)grd.x * 8 * 4)); GSR_TRY(c->hist.reserve(3 * HIST_BINS * 4));
        hipLaunchKernelGGL(k_prep, grd, blk, 0, st, n, L.xyz.as<float>(), L.color.as<float>(), L.cov6.as<float>(), L.opacity.as<float>(),
                           L.weight.as<float>(), L.is_parent.as<uint8_t>(), c->rec.as<float4>(), c->bbox_part.as<unsigned>(), (const long long*)nullptr);
        hipLaunchKernelGGL(k_bbox_reduce, dim3(1), dim3(256), 0, st, (int)grd.x, c->bbox_part.as<unsigned>(), c->bbox.as<unsigned>(),
                           (unsigned*)cnt, 16, c->hist.as<unsigned>(), 3 * HIST_BINS, (unsigned*)nullptr, 0);
        if (part) {     // the box of ALL ranks' components: maximum of the (order-preserving) codes, the minima complemented
            hipLaunchKernelGGL(k_flip3, dim3(1), dim3(64), 0, st, c->bbox.as<unsigned>());
            GSR_TRY(gsr_comm_allreduce(c->comm, c->bbox.p, 6, GSR_DT_U32, GSR_OP_MAX, (void*)st));
            hipLaunchKernelGGL(k_flip3, dim3(1), dim3(64), 0, st, c->bbox.as<unsigned>());
        }
        hipLaunchKernelGGL(k_hist, dim3(stride_grid(n) > 512 ? 512 : stride_grid(n)), blk, 0, st, n, L.xyz.as<float>(), c->bbox.as<unsigned>(), c->hist.as<unsigned>(),
                           (const long long*)nullptr);
        if (part) GSR_TRY(gsr_comm_allreduce(c->comm, c->hist.p, 3 * HIST_BINS, GSR_DT_U32, GSR_OP_SUM, (void*)st));      // integer counts: exact
        hipLaunchKernelGGL(k_grid_params, dim3(1), dim3(64), 0, st, c->bbox.as<unsigned>(), c->hist.as<unsigned>(), part ? c->n_global : n, c->cell_target,
                           c->max_cells, c->gparams.as<GridParams>(), (const long long*)nullptr);
        static_assert(sizeof(GridParams) == 40, "GridParams is read back as five 8-byte words");
        Collect q;
        q.n = 7;
        for (int i = 0; i < 5; ++i) { q.src[i] = (const char*)c->gparams.p + 8 * i; q.bytes[i] = 8; }
        q.src[5] = c->bbox.as<unsigned>() + 6; q.src[6] = c->bbox.as<unsigned>() + 7;      // k_prep's counts: parents, irregular components
        q.bytes[5] = q.bytes[6] = 4;
        unsigned long long w[8];
        GSR_TRY(read_back(c, q, w));
        memcpy(&gp, w, sizeof(gp));
        P_all = (int)(unsigned)w[5]; n_irr = (int)(unsigned)w[6];
    }
    overflow_flag = cnt + 12;
    c->stats[5] = gp.ncells;
    // The parents' output ranks depend on nothing but the level's flags (input order): flags as ints + their scan on the second
    // stream, beside the grid phase, instead of between the sums and the M-step (three launches off the critical path).
    GSR_TRY(c->pflag_in.reserve(n * 4)); GSR_TRY(c->oflag_in.reserve(n * 4)); GSR_TRY(c->prank_in.reserve(n * 4)); GSR_TRY(c->orank_in.reserve(n * 4));
    if (!part && c->aux && c->ev_pre) {
        GSR_HIP(hipEventRecord(c->ev_fork, st)); GSR_HIP(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
        hipLaunchKernelGGL(k_flags_in, grd, blk, 0, c->aux, n, n_own, L.is_parent.as<uint8_t>(), c->pflag_in.as<int>(), c->oflag_in.as<int>());
        GSR_TRY(exclusive_scan<int>(c, c->pflag_in.as<int>(), c->prank_in.as<int>(), n, true));
        GSR_HIP(hipEventRecord(c->ev_pre, c->aux));
        ranks_forked = true;
    }

    rec_src = c->rec.as<float4>();              // the packed records of the working set, by local index
    if (part) {
        GSR_TRY(pl.halo(gp, L, F, n));
        grd = dim3(stride_grid(n));
        rec_src = c->rec_loc.as<float4>();
    }
    GSR_TRY(c->keys.reserve(n * 4)); GSR_TRY(c->idx.reserve(n * 4)); GSR_TRY(c->skeys.reserve(n * 4)); GSR_TRY(c->order.reserve(n * 4));
    if (part) {
        // local components in ascending GLOBAL index (what a single GPU's input order is), then the stable sort by cell
        GSR_TRY(c->perm.reserve(n * 4));
        hipLaunchKernelGGL(k_iota, grd, blk, 0, st, n, c->idx.as<unsigned>());
        GSR_TRY(sort_pairs<unsigned>(c, c->gid_loc.as<unsigned>(), c->skeys.as<unsigned>(), c->idx.as<unsigned>(), c->perm.as<unsigned>(), n, bits_for(c->n_global + 1)));
        hipLaunchKernelGGL(k_keys_rec, grd, blk, 0, st, n, rec_src, c->perm.as<unsigned>(), c->gparams.as<GridParams>(), c->keys.as<unsigned>(), c->idx.as<unsigned>());
    } else
        hipLaunchKernelGGL(k_keys, grd, blk, 0, st, n, L.xyz.as<float>(), c->gparams.as<GridParams>(), c->keys.as<unsigned>(), c->idx.as<unsigned>());
    GSR_TRY(sort_pairs<unsigned>(c, c->keys.as<unsigned>(), c->skeys.as<unsigned>(), c->idx.as<unsigned>(), c->order.as<unsigned>(), n,
                                 bits_for(gp.ncells)));
    GSR_TRY(c->cellStart.reserve(((size_t)gp.ncells + 1) * 4));
    hipLaunchKernelGGL(k_run_starts<int>, grd, blk, 0, st, n, c->skeys.as<unsigned>(), (int64_t)gp.ncells, c->cellStart.as<int>());

    GSR_TRY(c->A.reserve((n + SEL_PAD) * 16)); GSR_TRY(c->geo.reserve((size_t)n * 64));
    if (sh_policy != 1) GSR_TRY(c->shs.reserve((size_t)n * (RSH > 0 ? RSH : 1) * 4));
    GSR_TRY(c->Rs.reserve(n * 4)); GSR_TRY(c->pflag.reserve(n * 4));
    GSR_TRY(c->iflag.reserve((n + 1) * 4)); GSR_TRY(c->irank.reserve((n + 1) * 4)); GSR_TRY(c->ipos.reserve(n * 4)); GSR_TRY(c->ppos.reserve(n * 4)); GSR_TRY(c->plist.reserve(n * 4));
    const bool tail = !part && F > 0;
    if (tail) GSR_TRY(c->sh_tail.reserve((size_t)(RSH + 4) * 4));
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((n + 255) / 256)), blk, 0, st, n, c->order.as<unsigned>(), rec_src, c->delta, c->A.as<float4>(), c->geo.as<float4>(),
                       c->Rs.as<float>(), c->pflag.as<int>(), c->iflag.as<int>(), L.sh.as<float>(), F, tail ? c->sh_tail.as<float>() : (float*)nullptr);
    // (a partitioned level: forked here -- the third stream carries the ghosts' SH rows, the gather queues up behind them; one GPU: behind
    // the selection, when the pair count that decides about the copy exists)
    if (part && F > 0) {
        hipLaunchKernelGGL(k_fill_const<int>, dim3(1), dim3(1), 0, st, (int64_t)1, reinterpret_cast<int*>(lvl + 3), 0);
        GSR_TRY(launch_gather_sh(true)); sh_launched = true;
    }
    GSR_TRY(exclusive_scan<int>(c, c->pflag.as<int>(), c->ppos.as<int>(), n));
    if (part) {     // the parents this rank works on are the ones it owns; the ghosts' parent flags still keep them out of the children's stream
        GSR_TRY(c->pown.reserve(n * 4)); GSR_TRY(c->ppos_own.reserve(n * 4)); GSR_TRY(c->inv.reserve(n * 4));
        hipLaunchKernelGGL(k_own_flags, grd, blk, 0, st, n, n_own, c->order.as<unsigned>(), c->pflag.as<int>(), c->pown.as<int>(), c->inv.as<unsigned>());
        GSR_TRY(exclusive_scan<int>(c, c->pown.as<int>(), c->ppos_own.as<int>(), n));
        hipLaunchKernelGGL(k_scatter_list, grd, blk, 0, st, n, c->pown.as<int>(), c->ppos_own.as<int>(), c->plist.as<unsigned>());
    } else
        hipLaunchKernelGGL(k_scatter_list, grd, blk, 0, st, n, c->pflag.as<int>(), c->ppos.as<int>(), c->plist.as<unsigned>());
    // the irregular components (never pre-rejected): their sorted positions, and their rank at every position
    // (a level without any -- k_prep counted them -- builds no list: pass B does not run then)
    if (part || n_irr > 0) {
        GSR_TRY(exclusive_scan<int>(c, c->iflag.as<int>(), c->irank.as<int>(), n + 1));
        hipLaunchKernelGGL(k_scatter_list, grd, blk, 0, st, n, c->iflag.as<int>(), c->irank.as<int>(), c->ipos.as<unsigned>());
    }
    P = P_all;                                  // (one GPU: the two counts came with the prologue, k_prep counted them)
    if (part) {
        Collect q;
        q.n = 5;
        q.src[0] = c->irank.as<int>() + n; q.src[1] = c->ppos.as<int>() + (n - 1); q.src[2] = c->pflag.as<int>() + (n - 1);
        q.src[3] = c->ppos_own.as<int>() + (n - 1); q.src[4] = c->pown.as<int>() + (n - 1);
        for (int i = 0; i < 5; ++i) q.bytes[i] = 4;
        unsigned long long w[8];
        GSR_TRY(read_back(c, q, w));
        n_irr = (int)w[0];
        P_all = (int)w[1] + (int)w[2];          // parents among the local components (they are no candidates)
        P = (int)w[3] + (int)w[4];              // parents this rank evaluates
    }
    c->stats[0] = P;
    c->stats_ex[0] = n_irr;
    // the candidate stream of pass A (non-parents only) and its prefix table
    GSR_TRY(c->Ac.reserve(((size_t)(n - P_all) + SEL_PAD) * 16)); GSR_TRY(c->cellStartC.reserve(((size_t)gp.ncells + 1) * 4));
    const bool have_irr = part || n_irr > 0;
    if (have_irr) GSR_TRY(c->cellStartI.reserve(((size_t)gp.ncells + 1) * 4));
    hipLaunchKernelGGL(k_child_stream, grd, blk, 0, st, n, (int64_t)gp.ncells, P_all, c->A.as<float4>(), c->pflag.as<int>(), c->ppos.as<int>(),
                       c->cellStart.as<int>(), c->Ac.as<float4>(), c->cellStartC.as<int>(), (int)SEL_PAD,
                       have_irr ? c->irank.as<int>() : (const int*)nullptr, c->cellStartI.as<int>());
    GSR_CHECKPOINT("grid + gather");
    GSR_TIME(c->ev[1], st);
    return GSR_OK;
}

// ---- 2. selection ------------------------------------------------------------------------------
// Fast path (SPARSE): one evaluation pass.  k_spans sums the span lengths per parent (an upper bound of
// its child count); every parent writes its pairs at the head of a segment of that capacity.  The sparse buffers cost 8 bytes per
// candidate scanned; when that exceeds the budget (GSR_HEM_SPARSE_GB, default 45 % of free HBM) the two-pass COUNT + FILL fallback
// runs instead (same device code, evaluates every candidate twice).  An asynchronous level takes the buffers as they are.
int32_t LevelRun::select_phase() {
    Pm = (size_t)(P > 0 ? P : 1);
    GSR_TRY(c->pcnt.reserve(Pm * 4)); GSR_TRY(c->pcap.reserve(Pm * 4)); GSR_TRY(c->poff.reserve((Pm + 1) * 8));
    GSR_TRY(c->scratch.reserve((Pm * 2 + 128) * 8));
    sa.A = c->A.as<float4>(); sa.geo = c->geo.as<float4>();
    sa.Rs = c->Rs.as<float>(); sa.plist = c->plist.as<unsigned>(); sa.cellStart = c->cellStart.as<int>();
    sa.gp = c->gparams.as<GridParams>(); sa.P = P;
    sa.Ac = c->Ac.as<float4>(); sa.cellStartC = c->cellStartC.as<int>(); sa.cellStartI = c->cellStartI.as<int>();
    sa.irank = c->irank.as<int>(); sa.ipos = c->ipos.as<unsigned>(); sa.n_irr = n_irr; sa.ell = c->use_ell ? 1 : 0;
    // work sharding: rank r of W evaluates the contiguous run [P r / W, P (r+1) / W) of the cell-sorted parents
    own_lo = sharded ? (int)((int64_t)P * c->shard_rank / c->shard_world) : 0;
    own_hi = sharded ? (int)((int64_t)P * (c->shard_rank + 1) / c->shard_world) : P;
    sa.own_lo = own_lo; sa.own_hi = own_hi;
    {   // colour gate  sqrtf(x) > kappa^2/2  (mixture.cpp:123) as a test on x: sqrtf is correctly rounded and monotone, so the
        // gate is  x > x*,  x* = the largest float whose square root does not exceed the threshold
        const float t = c->kappa * c->kappa * 0.5f;
        float x;
        if (t != t) x = t;                               // NaN threshold: never rejects
        else if (t < 0.0f) x = -1.0f;                    // every distance exceeds it
        else if (t > FLT_MAX) x = t;                     // +inf: never rejects
        else {
            x = t * t;
            if (x > FLT_MAX) x = FLT_MAX;
            while (x < FLT_MAX && sqrtf(nextafterf(x, INFINITY)) <= t) x = nextafterf(x, INFINITY);
            while (x > 0.0f && sqrtf(x) > t) x = nextafterf(x, -INFINITY);
        }
        sa.colorThr2 = x;
    }
    sa.kldThr = c->delta * c->delta * 0.5f;       // mixture.cpp:128
    sa.tau2 = c->tau * c->tau;                    // mixture.cpp:58,61
    sa.pcnt = c->pcnt.as<unsigned>();
    sa.pcap = c->pcap.as<unsigned>();
    sa.part_p = reinterpret_cast<const unsigned*>(lvl + 2);
    sa.abort_p = cnt + 2;
    // parents per selection wave: SEL_NP, but no fewer waves than the chip holds at once (256 CUs x 28)
    sa.np = c->select_np > 0 ? c->select_np : (P >= SEL_NP * 7168 ? SEL_NP : (P >= 2 * 7168 ? 2 : 1));
    M = 0;
    constexpr int WPB = SEL_WPB;
    // (the queue-serving kernel runs beside the light parents' on the context's second stream: launch_select forks / joins by events)
#define GSR_LAUNCH_SELECT(MODE) GSR_TRY(launch_select(MODE, sa, st, c->aux, c->ev_fork, c->ev_join))
    c->sparse_path = false;
    if (P > 0) {
        GSR_TRY(c->prec.reserve(Pm * sizeof(ParentRec)));
        launch_parent_prep(st, P, c->plist.as<unsigned>(), c->geo.as<float4>(), c->Rs.as<float>(), sa.kldThr, sa.ell, c->prec.as<ParentRec>());
        sa.prec = c->prec.as<ParentRec>();
        if (c->use_rowlist && Pm * 2 * SEL_ROWS * sizeof(int2) <= c->rowlist_max) {
            GSR_TRY(c->rowlist.reserve(Pm * 2 * SEL_ROWS * sizeof(int2)));
            sa.rowlist = c->rowlist.as<int2>();
        }
        launch_spans(st, sa);                                                         // candidates scanned per parent
        GSR_TRY(c->coff.reserve((Pm + 1) * 8));
        GSR_TRY(widen_scan(c->pcap.as<unsigned>(), c->coff.as<int64_t>(), P));
        // what the pair buffers hold today: an asynchronous level runs on that (k_select clamps every segment to it)
        cap_pairs = (unsigned long long)(std::min(c->sp_child.cap, c->sp_wl.cap) / 4);
        if (!spec) {
            int64_t cand_i = 0;
            GSR_TRY(total_of(c->coff.as<int64_t>(), c->pcap.as<unsigned>(), P, &cand_i));
            cand = (unsigned long long)cand_i;
            c->stats[4] = (int64_t)cand;
        }
        // processing order: heavy parents first (LPT), the light ones along a Z-order curve
        GSR_TRY(c->porder.reserve(Pm * 4)); GSR_TRY(c->pkeys.reserve(Pm * 4)); GSR_TRY(c->pkeys2.reserve(Pm * 4)); GSR_TRY(c->pidx.reserve(Pm * 4));
        {
            // "heavy" = 16x the mean capacity: k_heavy_keys takes the total from the scan itself
            hipLaunchKernelGGL(k_heavy_keys, dim3(stride_grid(P)), blk, 0, st, P, c->pcap.as<unsigned>(), c->coff.as<int64_t>(), c->plist.as<unsigned>(),
                               c->A.as<float4>(), c->gparams.as<GridParams>(), c->pkeys.as<unsigned>(), c->pidx.as<unsigned>());
            GSR_TRY((sort_pairs<unsigned, order_cfg>(c, c->pkeys.as<unsigned>(), c->pkeys2.as<unsigned>(), c->pidx.as<unsigned>(), c->porder.as<unsigned>(), P, order_key_bits(P) + 2)));
            if (!c->split_heavy)
                hipLaunchKernelGGL(k_count_heavy, dim3(1), dim3(1), 0, st, P, c->pkeys2.as<unsigned>(), cnt + 8);
            sa.porder = c->porder.as<unsigned>();
            sa.xcd = 1;
            sa.nheavy = cnt + 8;
            // work items of the heavy parents: sum(ceil(cap / part)) <= candidates / part + P, part >= 2048 (k_heavy_items chooses it)
            if (c->split_heavy) {
                const unsigned long long cand_bound = spec ? cap_pairs : cand;
                const int max_items = (int)std::min<unsigned long long>(cand_bound / 2048ull + (unsigned long long)P + 1ull, 0x7fffffffull);
                GSR_TRY(c->hitem.reserve((size_t)max_items * sizeof(uint2))); GSR_TRY(c->hfirst.reserve(Pm * 4));
                GSR_TRY(c->part_cnt.reserve((size_t)max_items * 4));
                sa.heavy_blocks = SEL_HEAVY_BLOCKS;
                sa.hitem = c->hitem.as<uint2>(); sa.hfirst = c->hfirst.as<int>(); sa.part_cnt = c->part_cnt.as<unsigned>();
                sa.hq = cnt + 10;
                hipLaunchKernelGGL(k_heavy_items, dim3(1), dim3(1024), 0, st, P, c->pkeys2.as<unsigned>(), cnt + 8, sa.porder,
                                   c->pcap.as<unsigned>(), c->coff.as<int64_t>(), reinterpret_cast<unsigned*>(lvl + 2), own_lo, own_hi,
                                   SEL_HEAVY_BLOCKS * WPB, max_items, c->hitem.as<uint2>(), c->hfirst.as<int>(), c->pcnt.as<unsigned>(), sa.hq,
                                   cnt + 13);
            }
        }
        bool sparse = true;
        if (!spec) {
            // the budget question needs the driver (hipMemGetInfo: a system call per level) only when the buffers would have to grow
            const char* sparse_env = getenv("GSR_HEM_SPARSE_GB");
            sparse = cand < (1ull << 40);
            if (sparse && (sparse_env || (size_t)cand * 4 > c->sp_child.cap || (size_t)cand * 4 > c->sp_wl.cap)) {
                size_t free_b = 0, total_b = 0;
                (void)hipMemGetInfo(&free_b, &total_b);
                size_t budget = (free_b + c->sp_child.cap + c->sp_wl.cap) / 20 * 9;      // 45 % of what is free (a 40 M-splat level needs 79 GB)
                if (sparse_env) budget = (size_t)(atof(sparse_env) * 1073741824.0);
                sparse = (double)cand * 8.0 <= (double)budget;
            }
        }
        if (sparse) {
            if (!spec) {
                const size_t Cm = (size_t)(cand > 0 ? cand : 1);
                GSR_TRY(c->sp_child.reserve(Cm * 4)); GSR_TRY(c->sp_wl.reserve(Cm * 4));
                cap_pairs = (unsigned long long)(std::min(c->sp_child.cap, c->sp_wl.cap) / 4);
            }
            sa.cap_pairs = cap_pairs;
            sa.poff = c->coff.as<int64_t>(); sa.pair_child = c->sp_child.as<unsigned>(); sa.pair_wl = c->sp_wl.as<float>();
            GSR_TIME1(c->evk[2], st);
            GSR_CHECKPOINT("spans + ordering");
            GSR_LAUNCH_SELECT(SEL_SPARSE);
            GSR_CHECKPOINT("k_select<SPARSE>");
            GSR_TIME1(c->evk[3], st);
        } else {
            GSR_TIME1(c->evk[0], st);
            GSR_LAUNCH_SELECT(SEL_COUNT);
            GSR_TIME1(c->evk[1], st);
        }
        GSR_TRY(widen_scan(c->pcnt.as<unsigned>(), c->poff.as<int64_t>(), P));
        if (!spec) GSR_TRY(total_of(c->poff.as<int64_t>(), c->pcnt.as<unsigned>(), P, &M));
        // the pairs stay where the selection wrote them (segments of capacity pcap[p] at coff[p]): the partition pass and the
        // M-step walk the segments.  Only the parts of the split parents are slid together (in place) -- by a handful of workgroups
        // in a chain of dependent copies, BEFORE the SH copy is let loose beside it: under that kernel's 5 TB/s the chain took 0.13 ms
        // of the 5 M level's critical path.
        if ((spec || M > 0) && sparse && sa.heavy_blocks)
            hipLaunchKernelGGL(k_join_parts, dim3(1024), blk, 0, st, sa.nheavy, sa.porder, c->coff.as<int64_t>(), sa.hfirst, sa.part_cnt,
                               c->pcap.as<unsigned>(), sa.part_p, c->sp_child.as<unsigned>(), c->sp_wl.as<float>());
        // the cell-sorted copy of the SH block -- if the level's pair count says it pays (k_gather_sh) -- on the third stream, beside the
        // pair partition and the per-child sums; joined in front of the M-step
        if (!sh_launched) { GSR_TRY(launch_gather_sh(c->aux2 != nullptr)); sh_launched = true; }
        if (spec || M > 0) {
            if (!sparse) {
                const size_t Mm = (size_t)(M > 0 ? M : 1);
                GSR_TRY(c->pair_child.reserve(Mm * 4)); GSR_TRY(c->pair_wl.reserve(Mm * 4));
                sa.poff = c->poff.as<int64_t>(); sa.pair_child = c->pair_child.as<unsigned>(); sa.pair_wl = c->pair_wl.as<float>();
                if (sa.heavy_blocks)                         // the queue cursor back behind the statically assigned items
                    hipLaunchKernelGGL(k_fill_const<int>, dim3(1), dim3(1), 0, st, (int64_t)1, sa.hq + 1, (int)(SEL_HEAVY_BLOCKS * WPB));
                GSR_TIME1(c->evk[2], st);
                GSR_LAUNCH_SELECT(SEL_FILL);
                GSR_TIME1(c->evk[3], st);
            }
        }
        c->sparse_path = sparse;
        c->stats_ex[1] = sparse ? 1 : 0;
    } else if (spec) {
        return GSR_RETRY_SYNC;                  // (a level without a parent: nothing to speculate about)
    }
#undef GSR_LAUNCH_SELECT
    c->stats[1] = M;
    GSR_CHECKPOINT("selection");
    GSR_TIME(c->ev[2], st);
    return GSR_OK;
}

// a compact copy of the pair list: only the exact partition (histogram + scan) and the sort path read one
int32_t LevelRun::compact_pairs() {
    if (!c->sparse_path) return GSR_OK;
    const size_t Mm = (size_t)(M > 0 ? M : 1);
    GSR_TRY(c->pair_child.reserve(Mm * 4)); GSR_TRY(c->pair_wl.reserve(Mm * 4));
    hipLaunchKernelGGL(k_compact_pairs, dim3(ceil_div(P, 8)), blk, 0, st, P, c->coff.as<int64_t>(), c->pcnt.as<unsigned>(), c->poff.as<int64_t>(),
                       (const int*)nullptr, (const unsigned*)nullptr, c->pcap.as<unsigned>(), (const unsigned*)nullptr, c->sp_child.as<unsigned>(), c->sp_wl.as<float>(),
                       c->pair_child.as<unsigned>(), c->pair_wl.as<float>());
    return GSR_OK;
}
// fixed-capacity partition: bucket regions of `cap` pairs (6x the mean, 8x on small levels; an asynchronous level: what the buffers hold),
// straight from the segments
int32_t LevelRun::sums_fixed() {
    unsigned cap;
    if (spec) {
        const size_t have = std::min(c->spair_child.cap / sizeof(slot_t), c->spair_wl.cap / 4) / (size_t)nbuckets;
        if (have < 4096) return GSR_RETRY_SYNC;
        cap = (unsigned)std::min<size_t>(have, 0xfffff000u);
    } else {
        const double mean = (double)M / (double)nbuckets;
        double capd = mean * (c->partition_factor > 0.0 ? c->partition_factor : (M < (1 << 24) ? 8.0 : 6.0)) + (c->partition_factor > 0.0 ? 64.0 : 4096.0);
        if (capd > 4.0e9) return GSR_E_INVALID;                  // (not an error: the caller takes the exact path)
        cap = (unsigned)capd;
        GSR_TRY(c->spair_child.reserve((size_t)nbuckets * cap * sizeof(slot_t))); GSR_TRY(c->spair_wl.reserve((size_t)nbuckets * cap * 4));
    }
    GSR_TRY(c->bcursor.reserve(((size_t)nbuckets + 1) * 8));
    if (sharded) GSR_HIP(hipMemsetAsync(c->bcursor.p, 0, ((size_t)nbuckets + 1) * 4, st));      // (one GPU: the level's prologue cleared the cursors, k_bbox_reduce)
    (void)hipGetLastError();
    GSR_TIME(c->evm[2], st);
    launch_partition(st, partition_mode(c), P, seg, c->pcnt.as<unsigned>(), pc, pw, nbuckets, bshift, cap, c->bcursor.as<unsigned>(),
                     c->spair_child.as<slot_t>(), c->spair_wl.as<float>(), overflow_flag);
    GSR_HIP(hipGetLastError());
    GSR_TIME(c->evm[3], st);
    GSR_CHECKPOINT("pair partition (fixed capacity)");
    GSR_TIME(c->evm[4], st);
    hipLaunchKernelGGL(k_bucket_sum, dim3(nbuckets), dim3(bshift >= 10 ? 1024 : 256), (size_t)12 << bshift, st, n, bshift, (const unsigned long long*)nullptr, cap,
                       c->bcursor.as<unsigned>(), c->spair_child.as<slot_t>(), c->spair_wl.as<float>(), c->sumLw.as<float>(), c->oflag.as<int>(),
                       c->geo.as<float>() + 15);
    GSR_TIME(c->evm[5], st);
    GSR_HIP(hipGetLastError());
    fixed_tried = true;
    return GSR_OK;
}
int32_t LevelRun::sums_exact() {
    // histogram + scan + scatter of a compact pair list, then one workgroup per bucket sums in LDS on a fixed-point scale.  The
    // partition kernels keep per-bucket counters in dynamic LDS (raised above the 64 KiB default in gsr_hem_create)
    const int tile = SUM_TILE;      // (x4 on levels with > 2000 buckets: measured, no gain)
    const int ntiles = (int)((M + tile - 1) / tile);
    GSR_TRY(compact_pairs());
    const size_t Mm = (size_t)(M > 0 ? M : 1);
    GSR_TRY(c->spair_child.reserve(Mm * 4)); GSR_TRY(c->spair_wl.reserve(Mm * 4));
    GSR_TRY(c->bhist.reserve(((size_t)nbuckets + 1) * 4)); GSR_TRY(c->bstart.reserve(((size_t)nbuckets + 1) * 8));
    GSR_TRY(c->bcursor.reserve(((size_t)nbuckets + 1) * 8));
    GSR_HIP(hipMemsetAsync(c->bhist.p, 0, ((size_t)nbuckets + 1) * 4, st));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_bucket_hist, dim3(ntiles), blk, (size_t)nbuckets * 4, st, M, tile, c->pair_child.as<unsigned>(), nbuckets, bshift, c->bhist.as<unsigned>());
    GSR_HIP(hipGetLastError());
    GSR_TRY(widen_scan(c->bhist.as<unsigned>(), (int64_t*)c->bstart.p, nbuckets + 1));
    GSR_HIP(hipMemcpyAsync(c->bcursor.p, c->bstart.p, ((size_t)nbuckets + 1) * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_bucket_scatter, dim3(ntiles), blk, (size_t)nbuckets * 4, st, M, tile, c->pair_child.as<unsigned>(),
                       c->pair_wl.as<float>(), nbuckets, bshift, c->bstart.as<unsigned long long>(), c->bcursor.as<unsigned long long>(),
                       c->spair_child.as<slot_t>(), c->spair_wl.as<float>());
    GSR_HIP(hipGetLastError());
    GSR_CHECKPOINT("pair partition");
    hipLaunchKernelGGL(k_bucket_sum, dim3(nbuckets), dim3(bshift >= 10 ? 1024 : 256), (size_t)12 << bshift, st, n, bshift, c->bstart.as<unsigned long long>(), 0u,
                       (const unsigned*)nullptr, c->spair_child.as<slot_t>(), c->spair_wl.as<float>(), c->sumLw.as<float>(), c->oflag.as<int>(),
                       c->geo.as<float>() + 15);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// ---- 3. per-child sums of wL (deterministic whatever the order: LDS fixed point, k_bucket_sum) ----------
// The pairs of parent p are the run [seg[p], seg[p] + pcnt[p]) of (pc, pw): the sparse segments of the one-pass selection or
// the compact CSR of the two-pass fallback.
int32_t LevelRun::sums_phase() {
    seg = c->sparse_path ? c->coff.as<int64_t>() : c->poff.as<int64_t>();
    pc = c->sparse_path ? c->sp_child.as<unsigned>() : c->pair_child.as<unsigned>();
    pw = c->sparse_path ? c->sp_wl.as<float>() : c->pair_wl.as<float>();
    GSR_TRY(c->cstart.reserve(((size_t)n + 1) * 8)); GSR_TRY(c->sumLw.reserve(n * 4)); GSR_TRY(c->oflag.reserve(n * 4));
    // children per bucket: SUM_BUCKET on large levels; on small ones fewer, so that the bucket kernel still has ~2 workgroups per CU
    bshift = SUM_BUCKET_SHIFT;
    while (bshift > 6 && (n >> bshift) < 512) --bshift;
    while (bshift < 13 && (n >> bshift) > 2500) ++bshift;       // very large levels: too many buckets scatter the partition's writes
    nbuckets = (int)((n + (1 << bshift) - 1) >> bshift);
    if (spec) {
        if (nbuckets > SUM_MAX_BUCKETS) return GSR_RETRY_SYNC;
        GSR_TRY(sums_fixed());
    } else if (part) {
        GSR_TRY(pl.sums(n, P, M, seg, pc, pw, nbuckets, bshift, overflow_flag));
    } else if (c->sum_bucket && M > 0 && nbuckets <= SUM_MAX_BUCKETS) {
        if (c->partition_fixed && !c->partition_overflowed) {
            const int32_t r = sums_fixed();
            if (r == GSR_E_INVALID && !fixed_tried) GSR_TRY(sums_exact()); else GSR_TRY(r);
        } else {
            if (c->partition_overflowed) c->stats_ex[2] = 1;
            GSR_TRY(sums_exact());
        }
    } else {
        if (M > 0) {
            GSR_TRY(compact_pairs());
            const size_t Mm = (size_t)M;
            GSR_TRY(c->spair_child.reserve(Mm * 4)); GSR_TRY(c->spair_wl.reserve(Mm * 4));
            GSR_TRY(sort_pairs<float>(c, c->pair_child.as<unsigned>(), c->spair_child.as<unsigned>(), c->pair_wl.as<float>(),
                                      c->spair_wl.as<float>(), M, bits_for(n)));
            GSR_CHECKPOINT("pair sort");
            hipLaunchKernelGGL(k_run_starts<int64_t>, dim3(stride_grid(M)), blk, 0, st, M, c->spair_child.as<unsigned>(), n, c->cstart.as<int64_t>());
        } else {
            hipLaunchKernelGGL(k_fill_const<int64_t>, grd, blk, 0, st, n + 1, c->cstart.as<int64_t>(), (int64_t)0);
        }
        GSR_TRY(c->spair_wl.reserve(4));
        hipLaunchKernelGGL(k_sumlw, dim3(stride_grid(n * 8)), blk, 0, st, n, c->cstart.as<int64_t>(), c->spair_wl.as<float>(), c->sumLw.as<float>(), c->oflag.as<int>(), c->geo.as<float>() + 15);
    }
    if (sharded) {
        // exchange 1: every rank holds the sums over ITS parents; the total decides responsibilities and orphans
        GSR_HIP(hipStreamSynchronize(st));
        if (c->shard_allreduce(c->sumLw.p, n, c->shard_user) != 0) return fail(GSR_E_INVALID, "gsr_hem_run_level: all-reduce callback failed (sumLw)");
        hipLaunchKernelGGL(k_orphan_flags, grd, blk, 0, st, n, c->sumLw.as<float>(), c->oflag.as<int>(), c->geo.as<float>() + 15);
    }
    GSR_CHECKPOINT("per-child sums");
    GSR_TIME(c->ev[3], st);
    return GSR_OK;
}

// ---- 4a. output ranks in input order: the orphans' flags back to input order, their scan, the level's row count ----------
int32_t LevelRun::output_ranks() {
    GSR_TRY(c->pflag_in.reserve(n * 4)); GSR_TRY(c->oflag_in.reserve(n * 4)); GSR_TRY(c->prank_in.reserve(n * 4)); GSR_TRY(c->orank_in.reserve(n * 4));
    int o_last = 0, o_flag = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (ranks_forked && attempt == 0) {
            GSR_HIP(hipStreamWaitEvent(st, c->ev_pre, 0));
        } else {
            hipLaunchKernelGGL(k_flags_in, grd, blk, 0, st, n, n_own, L.is_parent.as<uint8_t>(), c->pflag_in.as<int>(), c->oflag_in.as<int>());
            GSR_TRY(exclusive_scan<int>(c, c->pflag_in.as<int>(), c->prank_in.as<int>(), n));
        }
        hipLaunchKernelGGL(k_orphans_to_input_order, grd, blk, 0, st, n, c->order.as<unsigned>(), c->oflag.as<int>(), c->oflag_in.as<int>());
        GSR_TRY(exclusive_scan<int>(c, c->oflag_in.as<int>(), c->orank_in.as<int>(), n));
        if (spec) return GSR_OK;                    // (the counts stay on the device: k_level_tail, once the output's capacity is known)
        Collect q;
        q.n = 6;
        q.src[0] = c->orank_in.as<int>() + (n - 1); q.src[1] = c->oflag_in.as<int>() + (n - 1); q.src[2] = overflow_flag;
        q.src[3] = cnt + 13;
        q.src[4] = cnt + 8; q.src[5] = cnt + 10;      // heavy parents, their work items (statistics)
        for (int i = 0; i < 6; ++i) q.bytes[i] = 4;
        unsigned long long w[8];
        GSR_TRY(read_back(c, q, w));
        o_last = (int)w[0]; o_flag = (int)w[1];
        if (P > 0 && M >= 0 && c->stats[4] > 0) { c->stats_ex[3] = (int64_t)(unsigned)w[4]; c->stats_ex[4] = c->split_heavy ? (int64_t)(unsigned)w[5] : 0; }
        if (w[3] != 0ull) return fail(GSR_E_INVALID, "gsr_hem_run_level: the work-item table of the heavy parents overflowed (rerun with GSR_HEM_SPLIT=0)");
        if (!(fixed_tried && w[2] != 0ull) || attempt == 1) break;
        // a bucket region overflowed (pairs far more clustered than 6x the mean): the sums are incomplete.  Exact partition, and
        // this context stays with it
        c->partition_overflowed = true;
        c->stats_ex[2] = 1;
        GSR_HIP(hipMemsetAsync(overflow_flag, 0, 4, st));
        GSR_TRY(sums_exact());
        if (sharded) return fail(GSR_E_INVALID, "gsr_hem_run_level: bucket overflow on a sharded level");     // (sharded levels use the exact partition)
    }
    n_orph = (int64_t)o_last + o_flag;
    c->stats[2] = n_orph;
    n_pre = (int64_t)P + n_orph;
    return GSR_OK;
}

// ---- 4b. where the new level goes: the context's own arrays or the caller's (gsr_hem_set_output) ----------
int32_t LevelRun::open_output() {
    // rows the arrays must hold: n_pre -- or, for an asynchronous level, which does not know n_pre yet, the size of the level being reduced
    // (parents + orphans exceed it only when parents are orphans too: k_level_tail checks, the level then reruns)
    const int64_t need = spec ? n : n_pre;
    if (c->out_pending) {
        c->out_pending = false;                                 // one request, one level
        if (spec && P > c->out_rows) return GSR_RETRY_SYNC;     // (the synchronous level reports it)
        if (!spec && n_pre > c->out_rows) return fail(GSR_E_INVALID, "gsr_hem_run_level: the output arrays hold %lld rows, the level has %lld", (long long)c->out_rows, (long long)n_pre);
        if (F > 0 && !c->out_ptr[4]) return fail(GSR_E_INVALID, "gsr_hem_run_level: the output has no SH array but the level has F = %d", F);
        if (need > 0) {
            for (int i = 0; i < 5; ++i) {
                DevBuf* b = level_big(O, i);
                b->swap(c->spare_out[i]);
                b->borrow(c->out_ptr[i] ? c->out_ptr[i] : c->out_ptr[0]);       // reserve() on them is a no-op
            }
            out_active = true;
        }
    }
    GSR_TRY(O.reserve(need, F));
    out_cap = out_active ? std::min<int64_t>(c->out_rows, n + (int64_t)P) : need;     // (parents + orphans <= n + P)
    // an asynchronous level: O.weight / is_parent are the library's own arrays, reserved for `need` = n rows -- no row beyond them may be
    // written (a degenerate level whose parents are orphans too has more than n rows: k_level_tail raises the flag, the level reruns)
    if (spec) out_cap = std::min(out_cap, need);
    O.n = spec ? 0 : n_pre; O.F = F;
    if (spec)
        hipLaunchKernelGGL(k_level_tail, dim3(1), dim3(1), 0, st, n, P, c->orank_in.as<int>(), c->oflag_in.as<int>(), (long long)out_cap, lvl, cnt + 2);
    return GSR_OK;
}

// ---- 4c. M-step; orphans -----------------------------------------
int32_t LevelRun::mstep_phase() {
    const long long* n_pre_dev = spec ? lvl : nullptr;
    const int* sh_mode = reinterpret_cast<const int*>(lvl + 3);                     // where a child's SH row is read from: k_gather_sh decided
    // the new level's parent flags depend on nothing but the stream position and n_pre: drawn on the second stream beside the
    // M-step (the jump to the stream position is a fixed ~40 us chain, 5 % of a 200 k-splat level)
    rng_pos0 = c->rng_pos;
    const int64_t n_draw = spec ? out_cap : n_pre;
    if (!part && c->aux && n_draw > 0) {
        GSR_HIP(hipEventRecord(c->ev_fork, st)); GSR_HIP(hipStreamWaitEvent(c->aux, c->ev_fork, 0));
        GSR_TRY(O.is_parent.reserve((size_t)n_draw));
        GSR_TRY(draw_flags_raw(c, n_draw, O.is_parent.as<uint8_t>(), c->aux, n_pre_dev));
        GSR_HIP(hipEventRecord(c->ev_join, c->aux));
        flags_forked = true;
    }
    if (!sh_launched) { GSR_TRY(launch_gather_sh(false)); sh_launched = true; }                       // (a level without parents)
    if (sh_pending) { GSR_HIP(hipStreamWaitEvent(st, c->ev_sh_join, 0)); sh_pending = false; }      // the sorted SH rows are needed from here on
    if (P > 0) {
        MstepArgs ma;
        memset(&ma, 0, sizeof(ma));
        ma.geo = c->geo.as<float4>(); ma.RSH = RSH;
        ma.sh_mode_p = sh_mode; ma.sh_own = L.sh.as<float>(); ma.sh_sorted = c->shs.as<float>();
        ma.sh_last = part ? 0xffffffffu : (unsigned)(n - 1); ma.sh_tail = c->sh_tail.as<float>();
        ma.pair_child = pc; ma.pair_wl = pw;
        ma.P = P; ma.F = F;
        ma.small = c->mstep_small ? 1 : 0;
        // processing order: the selection's (heavy parents by candidates scanned first, then Z-order) -- parents with many
        // candidates are the ones with many pairs.  The per-parent headers are laid out in that order.
        const unsigned* mporder = (spec || M > 0) ? c->porder.as<unsigned>() : nullptr;
        ma.xcd = mporder ? 1 : 0;
        ma.nheavy = mporder ? cnt + 8 : nullptr;
        GSR_TRY(c->mhdr.reserve(Pm * sizeof(MstepHeader)));
        // heavy parents (more than MSTEP_SEG pairs): their segments are work items of a second launch (mstep_segment).  An asynchronous
        // level does not know whether there is one: the launch is always made (beside k_mstep, on the second stream) and finds its list empty
        const bool msplit = spec || M > MSTEP_SEG;              // (a parent of more than MSTEP_SEG pairs can exist)
        if (msplit) {
            const size_t Mb = (size_t)(spec ? cap_pairs : (unsigned long long)M);      // pairs <= candidates <= what the buffers hold
            const size_t cap_heavy = Mb / MSTEP_SEG + 2, cap_items = 2 * (Mb / MSTEP_SEG) + 4;
            GSR_TRY(c->mh_list.reserve(cap_heavy * sizeof(uint4))); GSR_TRY(c->mh_items.reserve(cap_items * sizeof(uint2)));
            GSR_TRY(c->mh_scratch.reserve(cap_items * (size_t)(16 + RSH) * 4));
        }
        unsigned* hcount = (unsigned*)cnt;                       // [0] heavy parents, [1] their segments (cleared with the level's counters)
        hipLaunchKernelGGL(k_mstep_headers, dim3(stride_grid(P)), blk, 0, st, P, mporder, c->plist.as<unsigned>(), seg,
                           c->pcnt.as<unsigned>(), c->order.as<unsigned>(), c->prank_in.as<int>(), c->A.as<float4>(), own_lo, own_hi,
                           c->mhdr.as<MstepHeader>(), (unsigned*)cnt + 15, (unsigned)MSTEP_SEG, msplit ? hcount : (unsigned*)nullptr,
                           c->mh_list.as<uint4>(), c->mh_items.as<uint2>());
        ma.hdr = c->mhdr.as<MstepHeader>();
        ma.split = c->mstep_split ? 1 : 0;
        ma.hcount = hcount; ma.hlist = c->mh_list.as<uint4>(); ma.hitems = c->mh_items.as<uint2>(); ma.hscratch = c->mh_scratch.as<float>();
        ma.o_xyz = O.xyz.as<float>(); ma.o_color = O.color.as<float>(); ma.o_cov6 = O.cov6.as<float>();
        ma.o_opacity = O.opacity.as<float>(); ma.o_weight = O.weight.as<float>(); ma.o_sh = O.sh.as<float>();
        // one wavefront per workgroup: consecutive parents on one CU share no cache lines in time (2 / 4 / 8 waves per workgroup
        // were measured 1 / 10 / 24 % slower)
        const int nq = RSH >> 2;                                // float4 per SH row; a lane covers MSTEP_NV of them
        // the heavy parents' segments: 2 048 waves pull them from the item table, on the second stream beside k_mstep when there is
        // one (the finish kernel adds a parent's segments in order); joined behind k_mstep
        hipStream_t hst = st;
        if (msplit && c->aux) {
            GSR_HIP(hipEventRecord(c->ev_mfork, st)); GSR_HIP(hipStreamWaitEvent(c->aux, c->ev_mfork, 0));
            hst = c->aux;
        }
#define GSR_LAUNCH_MSTEP(G)                                                                                              \
    {                                                                                                                    \
        if (msplit && hst != st) {                                                                                       \
            hipLaunchKernelGGL((k_mstep<G, 1, true>), dim3(2048), dim3(64), 0, hst, ma);                                 \
            hipLaunchKernelGGL(k_mstep_heavy_finish, dim3(256), dim3(64), 0, hst, ma);                                   \
            GSR_HIP(hipEventRecord(c->ev_mjoin, hst));                                                                   \
        }                                                                                                                \
        hipLaunchKernelGGL((k_mstep<G, 1>), dim3(8 * ceil_div(ceil_div(P, MSTEP_K), 8)), dim3(64), 0, st, ma);           \
        if (msplit && hst == st) {                                                                                       \
            hipLaunchKernelGGL((k_mstep<G, 1, true>), dim3(2048), dim3(64), 0, st, ma);                                  \
            hipLaunchKernelGGL(k_mstep_heavy_finish, dim3(256), dim3(64), 0, st, ma);                                    \
        }                                                                                                                \
    }
        GSR_TIME1(c->evm[0], st);
        if (nq == 0) { GSR_LAUNCH_MSTEP(0) }
        else if (nq <= 1 * MSTEP_NV) { GSR_LAUNCH_MSTEP(1) }
        else if (nq <= 2 * MSTEP_NV) { GSR_LAUNCH_MSTEP(2) }
        else if (nq <= 4 * MSTEP_NV) { GSR_LAUNCH_MSTEP(4) }
        else if (nq <= 8 * MSTEP_NV) { GSR_LAUNCH_MSTEP(8) }
        else if (nq <= 16 * MSTEP_NV) { GSR_LAUNCH_MSTEP(16) }
        else { GSR_LAUNCH_MSTEP(32) }      // F <= 384
#undef GSR_LAUNCH_MSTEP
        if (msplit && hst != st) GSR_HIP(hipStreamWaitEvent(st, c->ev_mjoin, 0));
        GSR_TIME1(c->evm[1], st);
    }
    hipLaunchKernelGGL(k_orphan_rows, dim3(stride_grid(n_own)), blk, 0, st, n_own, P, c->oflag_in.as<int>(), c->orank_in.as<int>(), L.xyz.as<float>(), L.color.as<float>(),
                       L.cov6.as<float>(), L.opacity.as<float>(), L.weight.as<float>(), L.sh.as<float>(), F, O.xyz.as<float>(), O.color.as<float>(),
                       O.cov6.as<float>(), O.opacity.as<float>(), O.weight.as<float>(), O.sh.as<float>(), (int64_t)(spec ? out_cap : n_pre));
    if (sharded && P > 0) {
        // exchange 2: the merged components.  Every rank packs the rows of ITS parents, ONE all-gather of equal chunks
        // (ceil(P / world) rows of 14 + F floats) moves them, and every rank scatters every chunk into the output rows
        // of the owners' slots: P (14 + F) 4 bytes per rank received in all, no floating-point arithmetic in the exchange.
        const int W = c->shard_world, RW = 14 + F;
        const int chunk = (P + W - 1) / W + 1;                    // rows per rank (the ranges differ by at most one)
        const size_t chunk_bytes = (size_t)chunk * RW * 4;
        GSR_TRY(c->shard_send.reserve(chunk_bytes)); GSR_TRY(c->shard_recv.reserve(chunk_bytes * W));
        const int own_cnt = own_hi - own_lo;
        if (own_cnt > 0)
            hipLaunchKernelGGL((k_shard_rows<true>), dim3(stride_grid((int64_t)own_cnt * RW)), blk, 0, st, own_lo, own_cnt, F, c->plist.as<unsigned>(),
                               c->order.as<unsigned>(), c->prank_in.as<int>(), c->shard_send.as<float>(), O.xyz.as<float>(), O.color.as<float>(),
                               O.cov6.as<float>(), O.opacity.as<float>(), O.weight.as<float>(), O.sh.as<float>());
        GSR_HIP(hipStreamSynchronize(st));
        if (c->shard_allgather(c->shard_send.p, c->shard_recv.p, (int64_t)chunk_bytes, c->shard_user) != 0)
            return fail(GSR_E_INVALID, "gsr_hem_run_level: all-gather callback failed (merged components)");
        for (int r = 0; r < W; ++r) {
            if (r == c->shard_rank) continue;
            const int lo = (int)((int64_t)P * r / W), hi = (int)((int64_t)P * (r + 1) / W);
            if (hi > lo)
                hipLaunchKernelGGL((k_shard_rows<false>), dim3(stride_grid((int64_t)(hi - lo) * RW)), blk, 0, st, lo, hi - lo, F, c->plist.as<unsigned>(),
                                   c->order.as<unsigned>(), c->prank_in.as<int>(), c->shard_recv.as<float>() + (size_t)r * chunk * RW, O.xyz.as<float>(),
                                   O.color.as<float>(), O.cov6.as<float>(), O.opacity.as<float>(), O.weight.as<float>(), O.sh.as<float>());
        }
    }
    P_glob = P; O_glob = n_orph;
    if (part) GSR_TRY(pl.global_ranks(P, n_pre, P_glob, O_glob));
    n_pre_glob = P_glob + O_glob;
    GSR_CHECKPOINT("M-step + orphans");
    GSR_TIME(c->ev[4], st);
    return GSR_OK;
}

// The validity erase in place, on the device (k_erase_save + k_erase_shift): lvl[0] = rows before it, cnt[3] / c->holes = what k_valid found;
// lvl[4] = rows after it.  Both kernels leave at once when there is nothing to erase -- or more than ERASE_MAX rows (the host's path then).
int32_t LevelRun::erase_in_place(int64_t rows_bound, bool may_allocate, int64_t alloc_rows) {
    // (the saved tails need 32 rows per tile of the bound -- 150 MB at 5 M rows -- and most clouds never erase a row: the buffer is allocated
    // the first time a level of this context does, by the host's path; until then an asynchronous level only COUNTS the erased rows.
    // alloc_rows: that first allocation covers the bound the ASYNCHRONOUS levels of this size will ask for -- the level's input size, not the
    // n_pre the host's path knows (sized for n_pre, every later asynchronous level found the buffer too small and took the
    // host's path again, a second round trip per surfel level))
    const int tile0 = std::min(256, 12288 / std::max(F, 6));
    const auto halo_bytes = [&](int64_t rows) { return (size_t)((rows + tile0 - 1) / tile0 + 1) * ERASE_MAX * ((size_t)(14 + F) * 4 + 1) + 64; };
    {
        const size_t need = halo_bytes(rows_bound);
        if (!may_allocate && c->erase_halo.cap < need) {
            hipLaunchKernelGGL(k_fill_const<long long>, dim3(1), dim3(1), 0, st, (int64_t)1, lvl + 4, (long long)0);     // (unused: the prologue reads lvl[0])
            return GSR_OK;
        }
    }
    erase_on_device = true;
    EraseArgs ea;
    memset(&ea, 0, sizeof(ea));
    float* arrs[6] = {O.xyz.as<float>(), O.color.as<float>(), O.cov6.as<float>(), O.opacity.as<float>(), O.weight.as<float>(), O.sh.as<float>()};
    const int ws[6] = {3, 3, 6, 1, 1, F};
    for (int q = 0; q < 6; ++q) { ea.arr[q] = arrs[q]; ea.w[q] = ws[q]; }
    ea.flags = O.is_parent.as<uint8_t>();
    ea.W = 14 + F;
    ea.tile = std::min(256, 12288 / std::max(F, 6));
    ea.max_tiles = (int)((rows_bound + ea.tile - 1) / ea.tile) + 1;
    GSR_TRY(c->erase_halo.reserve(halo_bytes(std::max(rows_bound, alloc_rows))));
    ea.halo = c->erase_halo.as<float>();
    ea.holes = c->holes.as<int>(); ea.dropped = cnt + 3; ea.n_pre_p = lvl; ea.n_keep_out = lvl + 4;
    const int g = std::min(ea.max_tiles, 2048);
    hipLaunchKernelGGL(k_erase_save, dim3(g), blk, 0, st, ea);
    hipLaunchKernelGGL(k_erase_shift, dim3(g), blk, (size_t)12288 * 4, st, ea);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

// the validity erase of a level that drops MANY rows (mixture.cpp:262-282): the surviving rows of every array move up, in order, through a second buffer
int32_t LevelRun::compact_erased(int64_t n_keep) {
    Level& T = c->tmp;
    const dim3 g2(stride_grid(n_pre));
    GSR_TRY(T.reserve(n_keep, F));
    T.n = n_keep; T.F = F;
    const int* keep = c->keep.as<int>();
    const int* pos = c->kpos.as<int>();
    hipLaunchKernelGGL(k_compact_rows, dim3(stride_grid(n_pre * 3)), blk, 0, st, n_pre, 3, keep, pos, O.xyz.as<float>(), T.xyz.as<float>());
    hipLaunchKernelGGL(k_compact_rows, dim3(stride_grid(n_pre * 3)), blk, 0, st, n_pre, 3, keep, pos, O.color.as<float>(), T.color.as<float>());
    hipLaunchKernelGGL(k_compact_rows, dim3(stride_grid(n_pre * 6)), blk, 0, st, n_pre, 6, keep, pos, O.cov6.as<float>(), T.cov6.as<float>());
    hipLaunchKernelGGL(k_compact_rows, g2, blk, 0, st, n_pre, 1, keep, pos, O.opacity.as<float>(), T.opacity.as<float>());
    hipLaunchKernelGGL(k_compact_rows, g2, blk, 0, st, n_pre, 1, keep, pos, O.weight.as<float>(), T.weight.as<float>());
    if (F > 0)
        hipLaunchKernelGGL(k_compact_rows4, dim3(stride_grid(n_pre * ((F + 3) / 4))), blk, 0, st, n_pre, F, keep, pos, O.sh.as<float>(), T.sh.as<float>());
    hipLaunchKernelGGL(k_compact_bytes, g2, blk, 0, st, n_pre, keep, pos, O.is_parent.as<uint8_t>(), T.is_parent.as<uint8_t>());
    if (out_active) {     // the caller's arrays stay the level's home: the compacted rows are copied back into them
        const size_t row_bytes[5] = {12, 12, 24, 4, (size_t)F * 4};
        for (int i = 0; i < 5; ++i)
            if (row_bytes[i] > 0 && n_keep > 0)
                GSR_HIP(hipMemcpyAsync(level_big(O, i)->p, level_big(T, i)->p, (size_t)n_keep * row_bytes[i], hipMemcpyDeviceToDevice, st));
        O.weight.swap(T.weight); O.is_parent.swap(T.is_parent);
        O.n = n_keep;
    } else
        O.swap(T);
    return GSR_OK;
}

// ---- 5. new parent flags (one draw per component, before the erase), validity erase (synchronous schedule) ---------
int32_t LevelRun::flags_and_validity() {
    if (part) {     // the libc stream is drawn for the GLOBAL level; a row takes the flag at its global rank
        GSR_TRY(c->allflags.reserve((size_t)(n_pre_glob > 0 ? n_pre_glob : 1)));
        GSR_TRY(draw_flags_raw(c, n_pre_glob, c->allflags.as<uint8_t>()));
        if (n_pre > 0)
            hipLaunchKernelGGL(k_gather_bytes, dim3(stride_grid(n_pre)), blk, 0, st, n_pre, c->gid_next.as<unsigned>(), c->allflags.as<uint8_t>(), O.is_parent.as<uint8_t>());
    } else if (flags_forked) {
        GSR_HIP(hipStreamWaitEvent(st, c->ev_join, 0));
    } else {
        GSR_TRY(draw_flags(c, O));
    }
    dropped = 0;
    if (n_pre > 0) {
        GSR_TRY(c->keep.reserve(n_pre * 4)); GSR_TRY(c->kpos.reserve(n_pre * 4));
        const dim3 g2(stride_grid(n_pre));
        GSR_TRY(c->holes.reserve(ERASE_MAX * 4));
        hipLaunchKernelGGL(k_valid, g2, blk, 0, st, n_pre, O.xyz.as<float>(), O.cov6.as<float>(), c->keep.as<int>(), (const long long*)nullptr, cnt + 3, c->holes.as<int>());
        if (part) GSR_TRY(exclusive_scan<int>(c, c->keep.as<int>(), c->kpos.as<int>(), n_pre));        // (drop_erased renumbers with it)
        {
            Collect q;
            q.n = 2;
            q.src[0] = cnt + 3; q.src[1] = cnt + 15;
            q.bytes[0] = q.bytes[1] = 4;
            unsigned long long w[8];
            GSR_TRY(read_back(c, q, w));
            dropped = (int64_t)(unsigned)w[0];
            if (P > 0) c->stats_ex[5] = (int64_t)(unsigned)w[1];
        }
        if (dropped > 0 && dropped <= ERASE_MAX && !part) {         // a handful of rows: in place, on the device
            hipLaunchKernelGGL(k_fill_const<long long>, dim3(1), dim3(1), 0, st, (int64_t)1, lvl, (long long)n_pre);
            GSR_TRY(erase_in_place(n_pre, true, n));
            O.n = n_pre - dropped;
        } else if (dropped > 0) {
            if (!part) GSR_TRY(exclusive_scan<int>(c, c->keep.as<int>(), c->kpos.as<int>(), n_pre));
            GSR_TRY(compact_erased(n_pre - dropped));
        }
    }
    n_glob_next = n_pre_glob;
    if (part) GSR_TRY(pl.drop_erased(O, n_pre, n_pre_glob, dropped, n_glob_next));
    GSR_CHECKPOINT("flags + validity");
    return GSR_OK;
}

int32_t LevelRun::run(int64_t* n_out, int64_t* n_dropped) {
    memset(c->stats, 0, sizeof(c->stats));
    memset(c->stats_ex, 0, sizeof(c->stats_ex));
    memset(c->part_stats, 0, sizeof(c->part_stats));
    c->stats[6] = n;
    if (part) {
        // the rank-local preconditions of a partitioned level are AGREED ON before its first data collective (one all-reduce of a status
        // word): a rank that returned by itself would leave its peers in the next collective for ever
        pl.W = gsr_comm_world(c->comm); pl.me = gsr_comm_rank(c->comm);
        const unsigned code = c->shard_world > 1 ? 4u : (pl.W > 8 ? 3u : (n >= (1ll << 30) ? 2u : 0u));
        GSR_TRY(pl.agree_on_preconditions(n, code));
    }
    if (n >= (1ll << 30)) return fail(GSR_E_INVALID, "gsr_hem_run_level: %lld components (the candidate records carry the sorted position in 30 bits)", (long long)n);
    if (n == 0) {
        if (n_out) *n_out = 0;
        if (n_dropped) *n_dropped = 0;
        return GSR_OK;
    }
    // An asynchronous level: one GPU, the default path of every stage, and buffers to run on (a fresh context's first level sizes them the
    // synchronous way).  What it cannot know beforehand it checks on the device (GSR_RETRY_SYNC).
    spec = spec && !part && !sharded && !dbg_sync && c->sum_bucket && c->partition_fixed && !c->partition_overflowed && c->partition_factor == 0.0 &&
           c->split_heavy && getenv("GSR_HEM_SPARSE_GB") == nullptr && c->aux != nullptr &&
           std::min(c->sp_child.cap, c->sp_wl.cap) >= (size_t)4096 && std::min(c->spair_child.cap / sizeof(slot_t), c->spair_wl.cap / 4) >= (size_t)4096;
    grd = dim3(stride_grid(n));
    GSR_TIME1(c->ev[0], st);
    GSR_TRY(grid_phase());
    GSR_TRY(select_phase());
    GSR_TRY(sums_phase());
    GSR_TRY(output_ranks());
    GSR_TRY(open_output());
    GSR_TRY(mstep_phase());

    unsigned long long w[LC_WORDS];
    bool have_next = false;             // w holds the next level's prologue
    const bool want_pro = !c->last_level;       // (the last level of a gsr_hem_run_levels hierarchy: nobody will read it)
    const int cb_next = c->cblock ^ 1;
    LevelCollect q;
    memset(&q, 0, sizeof(q));
    q.cnt = cnt; q.gp = c->gparams.as<GridParams>(); q.bbox = c->bbox.as<unsigned>();
    if (P > 0) { q.coff = c->coff.as<int64_t>(); q.pcap = c->pcap.as<unsigned>(); q.poff = c->poff.as<int64_t>(); q.pcnt = c->pcnt.as<unsigned>(); q.P = P; }
    if (spec) {
        // ---- 5 (asynchronous). flags joined, validity counted, the NEXT level's prologue on the rows as they are, ONE answer ----------
        if (flags_forked) GSR_HIP(hipStreamWaitEvent(st, c->ev_join, 0));
        GSR_TRY(c->keep.reserve((size_t)out_cap * 4)); GSR_TRY(c->kpos.reserve((size_t)out_cap * 4));
        GSR_TRY(c->holes.reserve(ERASE_MAX * 4));
        hipLaunchKernelGGL(k_valid, dim3(stride_grid(out_cap)), blk, 0, st, out_cap, O.xyz.as<float>(), O.cov6.as<float>(), c->keep.as<int>(), (const long long*)lvl, cnt + 3,
                           c->holes.as<int>());
        GSR_TRY(erase_in_place(out_cap, false));        // (leaves at once when nothing is erased; lvl[4] = the rows that remain)
        GSR_TIME1(c->ev[5], st);
        if (want_pro) GSR_TRY(enqueue_prologue(c, O, out_cap, erase_on_device ? lvl + 4 : lvl, cb_next));
        q.lvl = lvl;
        GSR_TRY(read_back_level(c, q, w));
        if (w[LC_FLAGS] != 0ull) return GSR_RETRY_SYNC;        // a clamped segment, a full bucket region or item table, an output too small
        cand = w[LC_CAND]; M = (int64_t)w[LC_PAIRS]; n_orph = (int64_t)w[LC_ORPHANS]; n_pre = (int64_t)w[LC_NPRE];
        c->stats[4] = (int64_t)cand; c->stats[1] = M; c->stats[2] = n_orph;
        c->stats_ex[3] = (int64_t)w[LC_HEAVY]; c->stats_ex[4] = (int64_t)w[LC_ITEMS]; c->stats_ex[5] = (int64_t)w[LC_MAXPAIRS];
        c->rng_pos = rng_pos0 + (uint64_t)n_pre;                // one draw per row of the new level (the launch covered a bound)
        O.n = n_pre;
        P_glob = P; O_glob = n_orph; n_pre_glob = n_pre; n_glob_next = n_pre;
        dropped = (int64_t)w[LC_DROPPED];
        have_next = dropped == 0 || (erase_on_device && dropped <= ERASE_MAX);      // (erased in place on the device: the prologue saw the level as it is now)
        if (have_next) O.n = n_pre - dropped;
        else if (dropped <= ERASE_MAX) {                // the first level of this context that erases rows: in place, from here (the buffer exists from now on)
            GSR_TRY(erase_in_place(n_pre, true, out_cap));
            O.n = n_pre - dropped;
        } else {                        // many rows to erase: the host finishes the level (scan + compaction), and the prologue is taken again
            GSR_TRY(exclusive_scan<int>(c, c->keep.as<int>(), c->kpos.as<int>(), n_pre));
            GSR_TRY(compact_erased(n_pre - dropped));
        }
    } else {
        GSR_TRY(flags_and_validity());
        GSR_TIME1(c->ev[5], st);
    }
    // the next level's prologue with this level's last round trip (one GPU); a partitioned / sharded level just waits for the stream
    if (!part && !sharded && !have_next && O.n > 0 && want_pro) {
        GSR_TRY(enqueue_prologue(c, O, O.n, nullptr, cb_next));
        GSR_TRY(read_back_level(c, q, w));
        have_next = true;
    } else if (!have_next) {
        GSR_HIP(hipStreamSynchronize(st));
    }
    unborrow_level0(c);                 // a borrowed level 0 goes back to the caller; cur gets its own buffers again
    c->cur.swap(c->nxt);
    if (out_active) {                   // the new current level lives in the caller's arrays: borrowed, its own buffers parked in spare
        out_active = false;
        for (int i = 0; i < 5; ++i) c->spare[i].swap(c->spare_out[i]);
        c->cur_borrowed = true;
    }
    if (have_next && want_pro && c->cur.n > 0) take_prologue(c, w, c->cur.n, cb_next); else c->pro.valid = false;
    if (part) { c->gid.swap(c->gid_next); c->n_global = n_glob_next; }
    c->stats[3] = dropped;
    c->stats[7] = c->cur.n;
    c->stats_ex[6] = c->round_trips;
    c->stats_ex[7] = spec ? 1 : 0;
    memset(c->phase_ms, 0, sizeof(c->phase_ms));
    memset(c->part_ms, 0, sizeof(c->part_ms));
    memset(c->kernel_ms, 0, sizeof(c->kernel_ms));
    if (c->timing >= 1) {
        if (c->timing >= 2) for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&c->phase_ms[i], c->ev[i], c->ev[i + 1]);
        (void)hipEventElapsedTime(&c->phase_ms[5], c->ev[0], c->ev[5]);
        c->phase_ms[5] += pro_ms;           // the level's time includes its prologue, wherever that ran
        if (c->timing >= 2) c->phase_ms[0] += pro_ms;
        c->phase_ms[6] = c->phase_ms[7] = 0.0f;
        if (P > 0 && !c->sparse_path) (void)hipEventElapsedTime(&c->phase_ms[6], c->evk[0], c->evk[1]);
        if (P > 0 && (M > 0 || c->sparse_path)) (void)hipEventElapsedTime(&c->phase_ms[7], c->evk[2], c->evk[3]);
        if (part && c->timing >= 2) {
            (void)hipEventElapsedTime(&c->part_ms[0], c->evp[0], c->evp[1]);
            if (F > 0) { GSR_HIP(hipStreamSynchronize(c->aux2)); (void)hipEventElapsedTime(&c->part_ms[1], c->evp[2], c->evp[3]); }
        }
        c->kernel_ms[0] = c->phase_ms[7];
        if (P > 0) (void)hipEventElapsedTime(&c->kernel_ms[1], c->evm[0], c->evm[1]);
        if (c->timing >= 2 && fixed_tried && !c->partition_overflowed) {
            (void)hipEventElapsedTime(&c->kernel_ms[2], c->evm[2], c->evm[3]);
            (void)hipEventElapsedTime(&c->kernel_ms[3], c->evm[4], c->evm[5]);
        }
    }
    if (n_out) *n_out = c->cur.n;
    if (n_dropped) *n_dropped = dropped;
    return GSR_OK;
}

}  // namespace
