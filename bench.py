#!/usr/bin/env python3
"""Benchmark of the hot path: HEM mixture levels + coarse-to-fine ICP on a synthetic splat pair.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--splats n] [--mode replicas|c4|c5] [--dump-outputs DIR] [--full [--no-cpu-baseline]]

One STEP = one pass of the whole hot path over one pair of clouds that is already resident in HBM:
  3 HEM levels on the source cloud and on the target cloud (rho=3, delta=3, kappa=2.5, tau=1 --
  src/params/merge_parameters.py:5-10), covariance normals for every level, then the 4-entry
  coarse-to-fine point-to-plane ICP (iter_values [50,30,20,10], max_corr [0.5,0.3,0.2,0.1]).
Workload at N=1 = BASELINE.json configs[2] (the configuration the metric is quoted on): 2 x 5M splats, SH degree 3.

Modes (one process per GPU, launched by torch.distributed.run for N > 1):
  replicas (default, what the driver measures)  every rank runs its own pair -- the path shards by independent clouds with
            no data-path collective (weak scaling); timing is barrier-bracketed and the MAX over ranks is taken.
  c4        BASELINE configs[3]: cloud A's HEM on rank 0, cloud B's on rank 1, the level lists exchanged once
            (broadcast), then ICP with the source split over ALL ranks and one RCCL all-reduce of the 32-double
            accumulator per iteration (strong scaling: the work is fixed).
  c5        BASELINE configs[4]: ONE large source cloud (--splats, 40 M on 8 GPUs) against a target of --target-splats
            (5 M): SPATIALLY PARTITIONED HEM levels -- every rank draws and keeps only its own block of the cloud
            (synth.make_block_cloud_torch), halo rows + integer partial sums per level through the library's communicator,
            the levels stay distributed --, ICP on every rank's piece with one all-reduce of 32 float64 per iteration.

A plain run does only what its headline figure needs: set-up, warm-up, the K timed steps, --dump-outputs if given, the line.
--full adds every side measurement (each outside the timed region, each a run of its own): one more pass of the levels with every
phase event on, the device-copy bandwidth, a single-level ICP on the full clouds, the surfel and clustered levels (--no-aniso
leaves them out), the CPU baseline (--no-cpu-baseline leaves it out) and, with --gpus N > 1, the strong-scaling children.

--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (float32 / float64, < 64 MB in all): every HEM
level's arrays and normals at a fixed, seeded sample of rows plus float64 column sums over all rows, the level sizes, and the ICP
result of every schedule entry.  The inputs depend on the arguments only, so two builds can be compared output for output.

With --gpus N > 1 in the default (replica) mode, --full also puts a "strong" object into the line: after the replica timing every rank
starts a CHILD process (same RANK / WORLD_SIZE, its own rendezvous port) that runs --mode c5 with 5 M x N splats (and --mode c4
when N = 2), under a host-side deadline; a hang, a crash or an RCCL error there ends up as {"error": ...} inside "strong" and can
never lose the replica line.  (A child process, not an exec: this process has initialised the GPU.)

Prints ONE JSON line on rank 0.  `value` = level-input Gaussians per second through the HEM levels (whole job);
`icp_iters_per_sec` rides along; `roofline` is for the dominant kernel of the step (algorithmic bytes of SURVEY.md 8(d));
`cpu_baseline` (--full) is the reference's own compiled extension (oracle/_ref) -- or the oracle port when that is absent --
timed on this box's host cores on a bounded ladder of sizes.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HEM_PARAMS = dict(hem_reduction=3.0, distance_delta=3.0, color_delta=2.5, decay_rate=1.0)
LEVELS = 3
ITER_VALUES = [50, 30, 20, 10]
MAX_CORR = [0.5, 0.3, 0.2, 0.1]
PAIR_ANGLE_DEG, PAIR_SHIFT_H = 5.0, 0.05      # rotation 5 degrees about (1,1,1)/sqrt(3), translation 0.05 h (1, -1, 0.5)
# configs[3]: the two clouds' HEM levels run on two GPUs at once, so cloud B cannot continue cloud A's rand() stream where A's levels end
# (qt_gaussian_mixture.py:55,79 does: one process, one stream).  Cloud k starts at position k * C4_STREAM_STRIDE of the same seed-1 stream
# (the device generator jumps ahead in O(log) steps).  Both from position 0 -- rounds 4-5 -- gave the synthetic pair, whose cloud B is cloud A
# moved with its rows in the same order, IDENTICAL parent flags: B's hierarchy was A's moved and the ICP converged in 50 / 2 / 1 / 1
# iterations instead of the 50 / 29 / 4 / 2 of the shared stream.
C4_STREAM_STRIDE = 1 << 40
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable copy rate)
# measured on MI355X (profiles/archive/r02_valu_issue_microbench.txt): cycles a SIMD needs per wave64 VALU instruction with >= 2 waves resident
VALU_CYCLES = {"full_rate (v_fma/mul/add/and/or with VGPR or constant operands)": 2.2,
               "half_rate (any SGPR operand, v_cmp, v_cndmask, v_bcnt/mbcnt, shifts, cvt, DPP, pk_*, f64)": 4.1,
               "transcendental": 8.1, "one wave alone": 4.9}


def bytes_level(n_in, n_out, F):
    """algorithmic bytes of one HEM level."""
    B = 57 + 4 * F
    return n_in * (B + 16) + n_out * B


def kernel_build_id():
    """Identifies the kernel sources a PMC summary belongs to (profiles/*_pmc.json carry it): the counter passes run
    scripts/prof_hem.py, the HEM level alone, so the HEM sources."""
    h = hashlib.sha256()
    for f in ("hem.hip", "hem_select.hip", "hem_select.h", "hem_device.h", "gsr_math.h", "gsr_common.h"):
        h.update(open(os.path.join(ROOT, "gaussiansplattingregistration_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def pmc_summary(kernel_prefix):
    """Counters of the dominant kernel from the newest committed PMC summary (profiles/*_pmc.json: separate
    `rocprofv3 --pmc` passes of scripts/prof_hem.py 5000000 1, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes
    for gfx950) -- only when that summary was taken with THESE kernel sources; otherwise (None, reason)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json")), key=os.path.basename)
    build = kernel_build_id()
    for f in reversed(files):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("kernel_build") != build:
            continue
        for k, v in d.items():
            if isinstance(v, dict) and k.startswith(kernel_prefix):
                return dict(v, source=os.path.basename(f)), None
    return None, "no profiles/*_pmc.json taken with the current kernel sources (kernel_build %s)" % build


def hem_levels(m, cloud, borrow=True, arenas=None, key=None, normals=False, raw=None):
    """3 HEM levels of one cloud on context m, ONE library call (gsr_hem_run_levels = MixtureCreator::CreateMixture, mixture_wrapper.cpp:10-18);
    returns (level list for ICP, per-level stats).  arenas / key: a dict that keeps this cloud's output arenas from step to step (no
    allocation in steady state).  normals: the levels' normals leave with the levels (computed on the library's side stream beside the next
    level) and level 0's with them -- the target side of point-to-plane ICP (point_cloud_converter.py:40-43).  raw: a dict that receives
    every level's arrays ("levels") and level 0's normals ("normals0") -- what --dump-outputs writes."""
    import torch
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    m.set_level0(cloud["xyz"], cloud["color"], cloud["opacity"], cloud["cov6"], cloud["sh"], borrow=borrow)     # resident in HBM: read in place
    n0 = int(cloud["xyz"].shape[0])
    arena = nrm0 = None
    if arenas is not None:
        arena = arenas.get((key, n0, normals))
        if arena is None:
            # LEVELS x n0 rows: always enough (a level never grows).  The isotropic cloud's three levels fill 0.48 n0 + room for level 3's input, the surfel
            # cloud's 1.6 n0 (its levels keep 60 - 90 % of their input: 1.5 n0 was too small, found by --workload aniso)
            arena = arenas[(key, n0, normals)] = m.new_arena(LEVELS * (n0 + 64), normals=normals)
            if normals:
                arena["normals0"] = torch.empty((n0, 3), dtype=torch.float64, device=arena["xyz"].device)
        nrm0 = arena.get("normals0")
    elif normals:
        arena = m.new_arena(LEVELS * (n0 + 64), normals=True)
        nrm0 = torch.empty((n0, 3), dtype=torch.float64, device=arena["xyz"].device)
    levels, stats = m.run_levels(LEVELS, arena=arena, normals0=nrm0)       # zero-copy: every level is written into the arena and read from it by the next
    if raw is not None:
        raw.update(levels=levels, normals0=nrm0)
    lv = [PointCloud(xyz32=cloud["xyz"], cov6=cloud["cov6"], normals=nrm0)]
    for d in levels:
        lv.append(PointCloud(xyz32=d["xyz"], cov6=d["cov6"], normals=d.get("normals")))
    return lv, stats


def coarse_to_fine(lru, ctx, clouds_src, clouds_tgt, device, sharded=None, comm=None, src_global_sizes=None, prepared=None):
    """4-entry coarse-to-fine ICP over the level lists (qt_multiscale_registrator.py:197-236).  sharded = (rank, world)
    splits every level's source over the ranks; src_global_sizes: the source levels ARE this rank's shards already (the pieces of
    a spatially partitioned HEM) and these are their sizes over all ranks.  comm: the library's communicator (RCCL enqueued by
    the library on the ICP context's stream); without it the torch.distributed trampoline of round 2.  prepared = one ICP context
    per entry (coarsest first) whose target index and normals were built already, beside the HEM levels (step_replicas)."""
    from gaussiansplattingregistration_amd import parallel
    T = np.eye(4)
    est = lru.get_estimation(lru.LocalRegistrationType.ICP_Point_To_Plane, lru.RobustLoss(0))
    out = {"icp_iters": 0, "levels": []}
    if src_global_sizes is None and not sharded and prepared is None:
        # the plain single-process schedule: ONE library call (gsr_icp_register_multiscale = the loop of qt_multiscale_registrator.py:197-236), no Python
        # between the entries
        entries = []
        for k in range(LEVELS + 1):
            s, t = clouds_src[-(k + 1)], clouds_tgt[-(k + 1)]
            if not t.has_normals():
                t.estimate_normals()
            entries.append((s.xyz32, t.xyz32, t.normals, MAX_CORR[k], ITER_VALUES[k]))
        res = ctx.register_multiscale(entries, T, est.kind, 0, 0.0, 1e-6, 1e-6)
        for e, r in zip(entries, res):
            out["icp_iters"] += r["iterations"]
            out["levels"].append({"ns": int(e[0].shape[0]), "nt": int(e[1].shape[0]), "iterations": r["iterations"], "ms_iters": r["ms_iters"],
                                  "evals": r["evaluations"], "ms_build": r["ms_build"],
                                  "T": r["transformation"], "fitness": r["fitness"], "rmse": r["inlier_rmse"]})
        out["T"], out["fitness"], out["rmse"] = res[-1]["transformation"], res[-1]["fitness"], res[-1]["inlier_rmse"]
        return out
    for k in range(LEVELS + 1):
        s, t = clouds_src[-(k + 1)], clouds_tgt[-(k + 1)]
        if not t.has_normals():
            t.estimate_normals()
        crit = lru.get_convergence_criteria(1e-6, 1e-6, ITER_VALUES[k])
        if src_global_sizes is not None:
            r = lru.registration_icp(s, t, MAX_CORR[k], T, est, crit, device=device, ctx=ctx, comm=comm, n_source_global=src_global_sizes[-(k + 1)])
        elif sharded:
            r = parallel.registration_icp_sharded(s, t, MAX_CORR[k], T, est, crit, sharded[0], sharded[1], device=device, ctx=ctx, comm=comm)
        elif prepared is not None:
            r = lru.registration_icp(s, t, MAX_CORR[k], T, est, crit, device=device, ctx=prepared[k], target_prepared=True)
        else:
            r = lru.registration_icp(s, t, MAX_CORR[k], T, est, crit, device=device, ctx=ctx)
        T = r.transformation
        out["icp_iters"] += r.iterations
        out["levels"].append({"ns": len(s), "nt": len(t), "iterations": r.iterations, "ms_iters": r.timing["ms_iters"],
                              "evals": r.timing["iter_kernels"], "ms_build": r.timing["ms_build"],
                              "T": r.transformation, "fitness": r.fitness, "rmse": r.inlier_rmse})
    out["T"], out["fitness"], out["rmse"] = T, r.fitness, r.inlier_rmse
    return out


def step_replicas(ctxs, lru, src, tgt, device, sync):
    """One pass over one pair on this rank.  `ctxs` holds the long-lived library contexts (their workspaces are reused
    from step to step: no allocation in steady state).

    Default (`serial` in ctxs): cloud 1 then cloud 2 on ONE context and one shared rand() stream (what a single reference process does,
    qt_gaussian_mixture.py:55,79), then the ICP.  --concurrent-clouds: the two clouds are independent, so their HEM
    levels run CONCURRENTLY -- two contexts on two
    streams driven by two host threads (the C ABI releases the GIL) -- and the thread of the target cloud also computes every
    level's normals as soon as that level exists (the ICP set-up hides behind the
    latency-bound small levels of the other cloud; the index BUILDS stay in the ICP phase, see main()).  Each cloud's parent flags are those of a fresh reference process (context-
    local rand() stream at position 0).  Measured and not made the default (see --concurrent-clouds in main())."""
    import threading
    import torch
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    out = {"hem_gaussians": 0, "kern": []}
    t0 = time.perf_counter()
    if ctxs.get("serial"):
        clouds, out["outputs"] = [], []
        m = ctxs["hem"]
        m.set_rng("glibc", 1, 0)                       # a fresh reference process: cloud 1 then cloud 2 on one stream
        for ci, c in enumerate((src, tgt)):
            raw = {}
            lv, st = hem_levels(m, c, arenas=ctxs.setdefault("arenas", {}), key=ci, normals=(ci == 1), raw=raw)       # the target's normals leave with its levels
            out["hem_gaussians"] += sum(s["n_in"] for s in st)
            out["kern"] += st
            clouds.append(lv)
            out["outputs"].append(raw)
        sync()
        t1 = time.perf_counter()
        out["hem_s"] = t1 - t0
        out["level_sizes"] = [len(p) for p in clouds[0]]
        out.update(coarse_to_fine(lru, ctxs["icp"], clouds[0], clouds[1], device))
        sync()
        out["icp_s"] = time.perf_counter() - t1
        return out
    res, err = {}, []

    def run_src():
        try:
            with torch.cuda.stream(ctxs["stream_a"]):
                ctxs["hem"].set_rng("glibc", 1, 0)
                res["src_raw"] = {}
                res["src"] = hem_levels(ctxs["hem"], src, raw=res["src_raw"])
                ctxs["stream_a"].synchronize()
        except BaseException as e:  # pragma: no cover
            err.append(e)

    def run_tgt():
        try:
            with torch.cuda.stream(ctxs["stream_b"]):
                m = ctxs["hem_b"]
                m.set_rng("glibc", 1, 0)

                def prepare(pc, j):                        # the level's normals (what the ICP phase would compute first), on this thread's stream
                    pc.estimate_normals()

                lv = [PointCloud(xyz32=tgt["xyz"], cov6=tgt["cov6"])]
                m.set_level0(tgt["xyz"], tgt["color"], tgt["opacity"], tgt["cov6"], tgt["sh"], borrow=True)
                stats, levels = [], []
                for j in range(1, LEVELS + 1):
                    m.run_level()
                    stats.append(m.stats())
                    d = m.get_level(as_torch=True)
                    levels.append(d)
                    lv.append(PointCloud(xyz32=d["xyz"], cov6=d["cov6"]))
                    prepare(lv[j], j)
                prepare(lv[0], 0)                          # the finest entry last: it is needed last
                ctxs["stream_b"].synchronize()
                res["tgt"] = (lv, stats)
                res["tgt_raw"] = {"levels": [dict(d, normals=p.normals) for d, p in zip(levels, lv[1:])], "normals0": lv[0].normals}
        except BaseException as e:  # pragma: no cover
            err.append(e)

    th = [threading.Thread(target=run_src), threading.Thread(target=run_tgt)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if err:
        raise err[0]
    sync()
    t1 = time.perf_counter()
    out["hem_s"] = t1 - t0
    for key in ("src", "tgt"):
        out["hem_gaussians"] += sum(s["n_in"] for s in res[key][1])
        out["kern"] += res[key][1]
    out["level_sizes"] = [len(p) for p in res["src"][0]]
    out["outputs"] = [res["src_raw"], res["tgt_raw"]]
    out.update(coarse_to_fine(lru, ctxs["icp"], res["src"][0], res["tgt"][0], device))
    sync()
    out["icp_s"] = time.perf_counter() - t1
    return out


def step_c4(ctxs, lru, src, tgt, device, sync, rank, world, comm=None):
    """configs[3]: cloud A's HEM on rank 0, cloud B's on rank 1 (no collective), one exchange of the level lists, ICP with
    the source split over all ranks and the accumulator all-reduce."""
    import torch
    import torch.distributed as dist
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    out = {"hem_gaussians": 0, "kern": []}
    t0 = time.perf_counter()
    mine = None
    if rank < 2:
        m = ctxs["hem"]
        m.set_rng("glibc", 1, rank * C4_STREAM_STRIDE)     # context-local stream: the two clouds are independent (C4_STREAM_STRIDE above)
        mine, st = hem_levels(m, src if rank == 0 else tgt)
        out["kern"] = st
        out["hem_gaussians"] = sum(s["n_in"] for s in st)
    sync()
    dist.barrier()
    t1 = time.perf_counter()
    out["hem_s"] = t1 - t0
    # exchange: every level of A (from rank 0) and of B (from rank 1) to every rank -- xyz and cov6 only, what ICP consumes
    dev = torch.device("cuda", device)
    nccl = dist.get_backend() == "nccl"

    def bcast(t, root):
        if nccl:
            dist.broadcast(t, root)
        else:
            h = t.cpu()
            dist.broadcast(h, root)
            t.copy_(h)

    lists = []
    for root in (0, 1):
        sizes = torch.tensor([len(p) for p in mine] if rank == root else [0] * (LEVELS + 1), dtype=torch.int64, device=dev)
        bcast(sizes, root)
        lv = []
        for k, n in enumerate(sizes.tolist()):
            if rank == root:
                xyz, cov = mine[k].xyz32.contiguous(), mine[k].cov6.contiguous()
            else:
                xyz, cov = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 6), dtype=torch.float32, device=dev)
            bcast(xyz, root)
            bcast(cov, root)
            lv.append(PointCloud(xyz32=xyz, cov6=cov))
        lists.append(lv)
    sync()
    t2 = time.perf_counter()
    out["exchange_s"] = t2 - t1
    out["level_sizes"] = [len(p) for p in lists[0]]
    out.update(coarse_to_fine(lru, ctxs["icp"], lists[0], lists[1], device, sharded=(rank, world), comm=comm))
    sync()
    out["icp_s"] = time.perf_counter() - t2
    out["outputs"] = [_pc_outputs(p) for p in lists]
    return out


def step_c5(lru, ctxs, blk, tgt, device, sync, rank, world, comm=None, owned=None, n_global=None):
    """configs[4]: one large source cloud against a smaller target.  The source's HEM levels are SPATIALLY PARTITIONED over the
    ranks (`blk` is this rank's block, `owned` its global indices; halo rows and integer partial sums through the library's
    communicator; the levels stay distributed); the target's levels are computed by every rank (it is the replicated side of the
    ICP); the ICP takes every rank's piece of a source level as its shard -- one all-reduce of 32 float64 per iteration."""
    from gaussiansplattingregistration_amd import hem, parallel
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    out = {"hem_gaussians": 0, "kern": []}
    t0 = time.perf_counter()
    if world > 1:
        pieces, st = parallel.hem_partitioned(blk, LEVELS, comm, device=device, as_torch=True, owned=owned, n_global=n_global, mixture=ctxs["hem"],
                                              rng_mode="glibc")
        src_list = [PointCloud(xyz32=blk["xyz"], cov6=blk["cov6"])] + [PointCloud(xyz32=p["xyz"], cov6=p["cov6"]) for p in pieces]
        sizes = [int(n_global)] + [int(s["n_global"]) for s in st]
        out["part"] = [{k: s_[k] for k in ("ghosts", "rows_sent", "halo_bytes_received", "sum_exchange_bytes_received", "n_global", "ms_halo_rows",
                                           "ms_halo_sh_overlapped", "ms_level")} for s_ in st]
    else:
        lv, st = hem.create_mixture(blk, LEVELS, device=device, as_torch=True, **HEM_PARAMS)
        src_list = [PointCloud(xyz32=blk["xyz"], cov6=blk["cov6"])] + [PointCloud(xyz32=l["xyz"], cov6=l["cov6"]) for l in lv]
        sizes = None
    out["kern"] += st
    out["hem_gaussians"] += sum(s["n_in"] for s in st)          # (rank-local level inputs; the global sizes ride in n_global)
    ctxs["hem2"].set_rng("glibc", 1, 0)
    tgt_list, stt = hem_levels(ctxs["hem2"], tgt)
    out["kern"] += stt
    # every rank computes the target's levels (the replicated side of the ICP): the job counts them once
    out["hem_gaussians_target_replicated"] = sum(s["n_in"] for s in stt)
    if rank == 0:
        out["hem_gaussians"] += out["hem_gaussians_target_replicated"]
    sync()
    t1 = time.perf_counter()
    out["hem_s"] = t1 - t0
    out["level_sizes"] = sizes if sizes is not None else [len(p) for p in src_list]
    out.update(coarse_to_fine(lru, ctxs["icp"], src_list, tgt_list, device, comm=comm, src_global_sizes=sizes))
    sync()
    out["icp_s"] = time.perf_counter() - t1
    out["outputs"] = [_pc_outputs(src_list), _pc_outputs(tgt_list)]          # (the source levels: this rank's pieces)
    return out


def _pc_outputs(pcs):
    """The arrays of a level list of PointClouds (level 0 = the input cloud: its normals only), as --dump-outputs takes them."""
    levels = []
    for p in pcs[1:]:
        d = {"xyz": p.xyz32, "cov6": p.cov6}
        if p.normals is not None:
            d["normals"] = p.normals
        levels.append(d)
    return {"levels": levels, "normals0": pcs[0].normals}


DUMP_ROWS = 16384          # rows of every level that --dump-outputs writes (a fixed, seeded sample; all rows of a smaller level)
DUMP_SEED = 2024
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(dirname, last):
    """--dump-outputs: what the LAST timed step computed, as dirname/<name>.npy in float32 / float64.  Per cloud (source, target) and
    level k = 1..3 every array the level carries at the same DUMP_ROWS rows (drawn with DUMP_SEED from the level's size, so two builds
    that agree on the sizes sample the same rows), and the float64 column sums of every array over ALL rows; level 0's normals likewise;
    the level sizes (one row per cloud); the ICP result of every schedule entry (coarsest first).  Returns the names written."""
    import torch
    os.makedirs(dirname, exist_ok=True)
    arrays = {"level_sizes": np.array([[int(lv["xyz"].shape[0]) for lv in raw["levels"]] for raw in last["outputs"]], dtype=np.float64)}

    def put(name, t):
        n = int(t.shape[0])
        rows = np.arange(n) if n <= DUMP_ROWS else np.sort(np.random.default_rng(DUMP_SEED + n).choice(n, DUMP_ROWS, replace=False))
        if isinstance(t, torch.Tensor):
            sample = t.index_select(0, torch.from_numpy(rows).to(t.device)).cpu().numpy()
            colsum = t.double().sum(0).cpu().numpy()
        else:
            t = np.asarray(t)
            sample, colsum = t[rows], t.astype(np.float64).sum(0)
        arrays[name] = sample if sample.dtype in (np.float32, np.float64) else sample.astype(np.float64)
        arrays[name + "_colsum"] = np.asarray(colsum, dtype=np.float64)

    for cloud, raw in zip(("source", "target"), last["outputs"]):
        if raw.get("normals0") is not None:
            put(f"{cloud}_level0_normals", raw["normals0"])
        for k, lv in enumerate(raw["levels"], start=1):
            for f, t in lv.items():
                if t is not None:
                    put(f"{cloud}_level{k}_{f}", t)
    ent = last["levels"]
    arrays["icp_transformation"] = np.asarray(last["T"], dtype=np.float64)
    arrays["icp_entry_transformations"] = np.stack([np.asarray(e["T"], dtype=np.float64) for e in ent])
    arrays["icp_entry_iterations_fitness_rmse"] = np.array([[e["iterations"], e["fitness"], e["rmse"]] for e in ent], dtype=np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte limit")
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return sorted(arrays)


def run_strong_children(a, rank, world, barrier):
    """The strong-scaling block of a multi-GPU replica run: BASELINE configs[3] (--mode c4, N = 2 only) and
    configs[4] (--mode c5 with --strong-splats x N splats) as CHILD processes of every rank, each with a host-side deadline.
    Returns (on rank 0) {"c5": {...}, "c4": {...}} -- the child's line condensed, or {"error": ...}.  Never raises."""
    base_port = int(os.environ.get("MASTER_PORT", "29500"))
    jobs = [("c5", ["--mode", "c5", "--splats", str(a.strong_splats * world), "--target-splats", str(a.strong_splats)])]
    if world == 2:
        jobs.append(("c4", ["--mode", "c4", "--splats", str(a.strong_splats)]))
    res = {}
    for k, (name, extra) in enumerate(jobs):
        port = base_port + 211 + 17 * k
        if port > 65000:
            port = base_port - 211 - 17 * k
        # the child's own rendezvous: RANK / WORLD_SIZE / LOCAL_RANK as here, a port of its own, and NOT the launcher's agent store
        env = {kk: v for kk, v in os.environ.items() if not kk.startswith("TORCHELASTIC_")}
        env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", str(a.strong_steps), "--warmup", "1", "--no-cpu-baseline",
               "--no-strong"] + extra
        t0 = time.perf_counter()
        r = {}
        try:
            with tempfile.TemporaryFile("w+") as err:
                p = subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, stderr=err, text=True)
                try:
                    out, _ = p.communicate(timeout=a.strong_timeout)
                except subprocess.TimeoutExpired:
                    p.kill()                                   # exactly the process started above
                    out, _ = p.communicate()
                    r["error"] = f"deadline of {a.strong_timeout:.0f} s passed (rank {rank}): the child was killed"
                if "error" not in r and p.returncode != 0:
                    err.seek(0)
                    r["error"] = f"child exited with {p.returncode}: " + err.read()[-400:].replace("\n", " | ")
            if "error" not in r and rank == 0:
                rows = [l for l in (out or "").splitlines() if l.startswith("{")]
                if not rows:
                    r["error"] = "the child printed no line"
                else:
                    d = json.loads(rows[-1])
                    r = {"workload": d["config"]["workload"], "parallelism": d["config"]["parallelism"], "level_sizes": d["config"]["level_sizes"],
                         "ms_per_step": d["ms_per_step"], "gaussians_per_s": d["value"], "hem_s_per_step": d["hem_s_per_step"],
                         "icp_s_per_step": d["icp_s_per_step"], "icp_iters_per_sec": d["icp_iters_per_sec"], "icp_iterations_per_step": d["icp_iterations_per_step"],
                         "T_err_vs_ground_truth_F": d["icp_result"]["T_err_vs_ground_truth_F"], "steps": d["steps"], "scaling": d["scaling"]}
                    for opt in ("partition_rank0", "exchange_s_per_step", "transport"):
                        if opt in d:
                            r[opt] = d[opt]
        except Exception as e:  # pragma: no cover
            r = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
        r["wall_s"] = time.perf_counter() - t0
        res[name] = r
        try:
            barrier()                                          # the parents meet again before the next job
        except Exception:  # pragma: no cover
            pass
    return res


def cpu_baseline(gpu_level1_rate, gpu_icp_coarse):
    """The reference's own extension (or the oracle port) on this box's host cores: one HEM level at 50 k / 200 k / 500 k / 1 M splats
    of the bench density with all cores (50 k and 200 k also with one thread), inside a time budget; ICP iterations per second of the
    oracle port on a 185 k-point level, tree build excluded.  gpu_level1_rate(n) -> the GPU's Gaussians/s for one level at
    the same n (measured here, same generator)."""
    from gaussiansplattingregistration_amd import synth
    from oracle import oracle as O
    cores = os.cpu_count() or 1
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    have_ref = os.path.isdir(ref_dir) and any(f.startswith("mixture_bind") for f in os.listdir(ref_dir))
    res = {"unit": "Gaussians/s", "cores": cores, "kind": "reference" if have_ref else "port", "ladder": []}
    budget_s, spent = 75.0, 0.0

    def run_one(n, threads):
        cloud = synth.make_cloud(n, seed=0)
        t_all = time.perf_counter()
        if have_ref:
            with tempfile.TemporaryDirectory() as td:
                inp, outp = os.path.join(td, "i.npz"), os.path.join(td, "o.npz")
                np.savez(inp, levels=1, rho=3.0, delta=3.0, kappa=2.5, tau=1.0, **{k: cloud[k] for k in ("xyz", "color", "opacity", "cov6", "sh")})
                subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "run_ref.py"), inp, outp, "--threads", str(threads)],
                               check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
                wall = float(np.load(outp)["wall_s"])
        else:
            t = time.perf_counter()
            O.hem(cloud, 1, threads=threads)
            wall = time.perf_counter() - t
        return wall, time.perf_counter() - t_all

    plan = [(50_000, cores), (50_000, 1), (200_000, cores), (200_000, 1), (500_000, cores), (1_000_000, cores)]
    for n, threads in plan:
        if spent > budget_s:
            res["ladder"].append({"n": n, "threads": threads, "skipped": "time budget"})
            continue
        try:
            wall, total = run_one(n, threads)
        except Exception as e:  # pragma: no cover
            res["ladder"].append({"n": n, "threads": threads, "error": str(e)[:120]})
            continue
        spent += total
        row = {"n": n, "threads": threads, "wall_s": wall, "gaussians_per_s": n / wall}
        if threads == cores:
            g = gpu_level1_rate(n)
            row["gpu_gaussians_per_s_same_n"] = g
            row["speedup"] = g / (n / wall)
        res["ladder"].append(row)
    full = [r for r in res["ladder"] if r.get("threads") == cores and "wall_s" in r]
    if full:
        top = max(full, key=lambda r: r["n"])
        res.update(value=top["gaussians_per_s"], speedup_like_for_like=top["speedup"],
                   sample=f"{'reference cpp_ext (oracle/_ref)' if have_ref else 'oracle port'} CreateMixture, 1 level, {top['n']} splats SH deg 3 at "
                          f"bench density, {cores} OpenMP threads, list marshalling excluded; wall {top['wall_s']:.2f} s; the GPU figure beside it is one "
                          "level of the SAME cloud")
    # ICP: the oracle port (Open3D absent) -- KD-tree ICP, point-to-plane, on a level of the size the coarsest bench level has;
    # iterations per second = extra iterations / extra time, so the tree build and the first evaluation cancel
    try:
        ns = 185000
        src, tgt, _ = synth.make_pair(ns, seed=1, sh_degree=0, angle_deg=1.0)
        C = tgt["cov6"].astype(np.float64)
        nrm = O.normals_from_cov(np.stack([C[:, [0, 1, 2]], C[:, [1, 3, 4]], C[:, [2, 4, 5]]], 1))
        t = time.perf_counter()
        O.icp(src["xyz"], tgt["xyz"], nrm, np.eye(4), kind=1, max_corr=0.5, max_iter=1, rel_fitness=0, rel_rmse=0, threads=cores)
        t1 = time.perf_counter() - t
        t = time.perf_counter()
        r = O.icp(src["xyz"], tgt["xyz"], nrm, np.eye(4), kind=1, max_corr=0.5, max_iter=11, rel_fitness=0, rel_rmse=0, threads=cores)
        t11 = time.perf_counter() - t
        rate = (r["iterations"] - 1) / max(1e-9, t11 - t1)
        res.update(icp_iters_per_sec=rate, icp_kind="port",
                   icp_sample=f"oracle KD-tree ICP (point-to-plane), {ns} x {ns} points, {cores} threads: 10 extra iterations took {t11 - t1:.2f} s "
                              f"(tree build + first evaluation {t1:.2f} s excluded)",
                   icp_gpu_iters_per_sec_same_size=gpu_icp_coarse, icp_speedup_like_for_like=(gpu_icp_coarse / rate) if gpu_icp_coarse else None)
    except Exception as e:  # pragma: no cover
        res["icp_error"] = str(e)[:120]
    # the bench's OWN size on the reference, measured once by hand (it takes 36 minutes on 256 cores: scripts/cpu_reference_5m.py) and
    # kept under profiles/ -- quoted here as what it is, not re-measured in this run
    try:
        ref5 = json.load(open(os.path.join(ROOT, "profiles", "archive", "r04_cpu_reference_5m.json")))
        res["reference_5m_measured_offline"] = {"source": "profiles/archive/r04_cpu_reference_5m.json (scripts/cpu_reference_5m.py, not part of this run)",
                                                "cores": ref5["cores"], "reference_wall_s_one_level": ref5["reference_wall_s"],
                                                "gpu_level_s_same_cloud": ref5["gpu_level_s"], "speedup_like_for_like": ref5["speedup_like_for_like"],
                                                "level_sizes_equal": ref5["level_sizes_equal"]}
    except Exception:
        pass
    return res


def main():
    global PAIR_ANGLE_DEG, PAIR_SHIFT_H
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)       # (the first step grows the contexts' buffers: 48 ms; the second is within 2 % of the steady state, scripts/steps_probe.py)
    ap.add_argument("--splats", "--n", dest="n", type=int, default=None, help="splats per cloud (c5: of the LARGE cloud); use --splats under torchrun")
    ap.add_argument("--target-splats", type=int, default=5_000_000, help="c5: splats of the target cloud")
    ap.add_argument("--mode", choices=["replicas", "c4", "c5"], default="replicas")
    ap.add_argument("--full", action="store_true", help="after the timed steps, every side measurement too (the phase pass, the copy bandwidth, the single-level "
                    "ICP, the surfel and clustered levels, the CPU baseline, with --gpus N > 1 the strong-scaling children); a plain run does only what the "
                    "headline figure needs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy (float32 / float64, a "
                    "fixed seeded sample of every level's rows, < 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--workload", choices=["iso", "aniso", "clustered"], default="iso",
                    help="splat shapes of the pair: SURVEY 8(d)'s isotropic recipe, or the surfel recipe (synth.make_cloud(shape='aniso'): 60 %% discs, "
                         "15 %% needles, covariance condition numbers 1e2 .. 1e5 on a smooth orientation field), or the large-scene recipe "
                         "(shape='clustered': 60 %% of the splats in 40 clumps of 30 .. 100 x the background density, giants, far outliers)")
    ap.add_argument("--no-aniso", action="store_true", help="--full: skip the anisotropic and clustered side measurements")
    ap.add_argument("--concurrent-clouds", action="store_true", help="replica mode: the two clouds' HEM levels side by side on two contexts / streams / host "
                    "threads (each cloud's rand() stream at position 0) and the target levels' normals computed in that phase, instead of cloud 1 then "
                    "cloud 2 on ONE context and one shared rand() stream (the default: what a single reference process does).  Measured (profiles/archive/r04c_*, "
                    "r04d_*): the HEM levels alone overlap to 27.0 instead of 28.9 ms in a bare harness, but the full step does not gain (37.7 - 43 ms "
                    "against 39.0): the two clouds' big kernels each fill the chip, and two Python threads add jitter")
    ap.add_argument("--no-strong", action="store_true", help="--full with --gpus N > 1, replica mode: skip the strong-scaling children (c5, and c4 at N = 2)")
    ap.add_argument("--strong-splats", type=int, default=5_000_000, help="strong block: splats per GPU of the c5 source (x N) and per cloud of c4")
    ap.add_argument("--strong-steps", type=int, default=2)
    ap.add_argument("--strong-timeout", type=float, default=300.0, help="host-side deadline of one strong child, seconds")
    a = ap.parse_args()
    if a.steps < 1:
        raise SystemExit("--steps must be at least 1")

    import torch
    import __graft_entry__ as g
    from gaussiansplattingregistration_amd import parallel
    rank, world, local_rank = parallel.init_distributed()
    if rank == 0:
        g.build_hip()                       # one rank (re)builds a stale library, the others wait for it
    if world > 1:
        torch.distributed.barrier()
    from gaussiansplattingregistration_amd import hem, icp as icp_mod, synth
    from gaussiansplattingregistration_amd.utils import local_registration_util as lru
    if a.gpus != world and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: this backend has no CPU fallback")
    if a.mode == "c4" and world < 2:
        raise SystemExit("--mode c4 needs at least 2 ranks (cloud A on rank 0, cloud B on rank 1)")
    device = local_rank if world > 1 else 0
    if os.environ.get("GSR_BENCH_SAME_DEVICE"):          # test hook: several ranks on one GPU (with GSR_DIST_BACKEND=gloo)
        device = 0
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)

    def sync():
        torch.cuda.synchronize(dev)

    def barrier():
        if world > 1:
            torch.distributed.barrier()

    # synthetic pair, resident in HBM before the timed region: target = cloud, source = inv(T_gt) * cloud + jitter
    n = a.n if a.n is not None else (40_000_000 if a.mode == "c5" else 5_000_000)
    seed = 100 + (rank if a.mode == "replicas" else 0)     # c4 / c5: every rank holds the same data (replicated inputs)
    owned = None
    if a.mode == "c5":
        # every rank draws ITS block of the large cloud and nothing else (the cloud is defined block by block: no rank ever holds or
        # sorts the 40 M splats); the target is a sub-sample of the same scene -- the first rows of every block, gathered ONCE onto
        # every rank (set-up, outside the timed region) -- moved by T_gt
        src, owned = synth.make_block_cloud_torch(n, rank, world, seed=seed, device=dev)
        # The c5 schedule (what runs, stated once).  Two scalings, both recorded in the line's config ("pair", "max_corr", "c5_scaling"):
        #   rel        the pair's motion relative to the 2 x 5 M pair's, so that the ratio of displacement to correspondence distance stays that pair's:
        #              a scene twice as wide (40 M) moved by the same 5 degrees displaces its corners twice as far (alone: rel = 0.5; measured at full
        #              size without it, profiles/r05a_bench_c5_40m_8ranks_one_gpu.json: fitness 0.59, T_err 0.76) ...
        #   corr_scale ... but the target is a SUB-SAMPLE of the scene, (n / nt)^(1/3) times the point spacing the schedule's correspondence distances
        #              were chosen for, so those grow by that factor and the motion with them: at 40 M against 5 M both factors are 2 and cancel --
        #              the pair moves by the full 5 degrees / 0.05 h with DOUBLED correspondence distances.  Lines of this mode are therefore not
        #              comparable with round 4's (fixed 0.5 ... 0.1).  (main() rebinds the module's MAX_CORR / PAIR_* for this process only.)
        rel = min(1.0, synth.half_extent(5_000_000) / src["h"])
        nt = min(a.target_splats, n)
        global MAX_CORR
        corr_scale = (n / nt) ** (1.0 / 3.0)
        MAX_CORR = [m_ * corr_scale for m_ in MAX_CORR]
        rel = min(1.0, rel * corr_scale)
        c5_scaling = {"corr_scale": corr_scale, "motion_rel": rel}
        PAIR_ANGLE_DEG, PAIR_SHIFT_H = PAIR_ANGLE_DEG * rel, PAIR_SHIFT_H * rel
        T_gt = synth.rigid_transform(PAIR_ANGLE_DEG, (1, 1, 1), PAIR_SHIFT_H * src["h"] * np.array([1.0, -1.0, 0.5]))
        fields = ("xyz", "color", "opacity", "cov6", "sh")
        parts = {f: [] for f in fields}
        for r in range(world):
            lo_r, hi_r = parallel.shard_range(nt, r, world)
            for f in fields:
                if r == rank:
                    t = src[f][:hi_r - lo_r].contiguous()
                else:
                    t = torch.empty((hi_r - lo_r,) + tuple(src[f].shape[1:]), dtype=torch.float32, device=dev)
                if world > 1:
                    if torch.distributed.get_backend() == "nccl":
                        torch.distributed.broadcast(t, r)
                    else:
                        hbuf = t.cpu()
                        torch.distributed.broadcast(hbuf, r)
                        t.copy_(hbuf)
                parts[f].append(t)
        sub = {f: torch.cat(parts[f]).contiguous() for f in fields}
        sub.update(sh_degree=src["sh_degree"], h=src["h"], shape=src["shape"])
        del parts
        tgt = synth.apply_rigid_torch(sub, T_gt)
        tgt = {k: (v.contiguous() if isinstance(v, torch.Tensor) else v) for k, v in tgt.items()}
    else:
        tgt = synth.make_cloud_torch(n, seed=seed, device=dev, shape=a.workload)
        if a.workload != "iso":
            # The surfel and the clustered clouds have no coarse level to speak of (thin discs merge with little: a level keeps 60-90 % of
            # its input; the clumps stay dense), and nearest-neighbour ICP from 5 degrees / 0.05 h apart does not leave the identity on
            # them (measured: T_err = |I - T_gt| after the whole budget).  Their step is run on a pair ICP can register: 1 degree, 0.01 h.
            PAIR_ANGLE_DEG, PAIR_SHIFT_H = 1.0, 0.01
        T_gt = synth.rigid_transform(PAIR_ANGLE_DEG, (1, 1, 1), PAIR_SHIFT_H * tgt["h"] * np.array([1.0, -1.0, 0.5]))
        src = synth.apply_rigid_torch(tgt, np.linalg.inv(T_gt))
        gen = torch.Generator(device=dev).manual_seed(7 + (rank if a.mode == "replicas" else 0))
        src["xyz"] = src["xyz"] + torch.randn(src["xyz"].shape, device=dev, generator=gen) * 0.002
        src = {k: (v.contiguous() if isinstance(v, torch.Tensor) else v) for k, v in src.items()}
    sync()

    if a.mode == "replicas" and a.concurrent_clouds:
        # two HEM contexts on two streams (the two clouds side by side); the target cloud's thread also computes every level's normals.
        # (Measured and not kept, profiles/archive/r04c_*: one ICP context per schedule entry with its target index built in that thread too --
        # the step fell from 38.97 to 37.7 ms, but the ICP iterations on the early-built indices ran 6-20 % slower and the HEM phase, with
        # the index builds inside it, rose from 29.4 to 32.5 ms: the headline rate fell by 9 %.)
        sa_, sb_ = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        ctxs = {"stream_a": sa_, "stream_b": sb_,
                "hem": hem.HemMixture(device=device, rng_mode="glibc", stream=sa_.cuda_stream, **HEM_PARAMS),
                "hem_b": hem.HemMixture(device=device, rng_mode="glibc", stream=sb_.cuda_stream, **HEM_PARAMS),
                "icp": icp_mod.IcpContext(device=device)}
    else:
        ctxs = {"hem": hem.HemMixture(device=device, rng_mode="glibc", **HEM_PARAMS), "icp": icp_mod.IcpContext(device=device), "serial": True}
    # the data-path collectives of c4 / c5 go through the LIBRARY's communicator: RCCL (nccl backend) enqueued by the library on its
    # own streams, or the callback transport (gloo: test boxes where the ranks share a GPU)
    from gaussiansplattingregistration_amd.comm import Comm
    comm = Comm.from_torch_group(device) if (world > 1 and a.mode in ("c4", "c5")) else None
    if a.mode == "c5":
        ctxs["hem2"] = hem.HemMixture(device=device, rng_mode="glibc", **HEM_PARAMS)       # the replicated target's levels

    def one_step():
        if a.mode == "c4":
            return step_c4(ctxs, lru, src, tgt, device, sync, rank, world, comm=comm)
        if a.mode == "c5":
            return step_c5(lru, ctxs, src, tgt, device, sync, rank, world, comm=comm, owned=owned, n_global=n)
        return step_replicas(ctxs, lru, src, tgt, device, sync)

    for _ in range(a.warmup):
        one_step()
    sync(); barrier()
    t0 = time.perf_counter()
    runs, last_outputs = [], None
    for _ in range(a.steps):
        r = one_step()
        o = r.pop("outputs")
        if a.dump_outputs:                  # the arrays of the last step only, and only for --dump-outputs
            last_outputs = o
        del o
        runs.append(r)
    sync(); barrier()
    elapsed = time.perf_counter() - t0
    hem_s, icp_s = sum(r["hem_s"] for r in runs), sum(r["icp_s"] for r in runs)
    hem_gauss = sum(r["hem_gaussians"] for r in runs)
    if world > 1:
        rdev = dev if torch.distributed.get_backend() == "nccl" else torch.device("cpu")
        t = torch.tensor([elapsed, hem_s, icp_s], dtype=torch.float64, device=rdev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed, hem_s, icp_s = (float(v) for v in t)
        tg = torch.tensor([float(hem_gauss)], dtype=torch.float64, device=rdev)
        torch.distributed.all_reduce(tg, op=torch.distributed.ReduceOp.SUM)
        # every rank's level inputs are different work (c5: the slabs of the partitioned source; the replicated target levels are
        # counted once, by rank 0)
        hem_gauss = float(tg)
    icp_iters = sum(r["icp_iters"] for r in runs) * (world if a.mode == "replicas" else 1)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, dict(runs[-1], outputs=last_outputs))
    del last_outputs

    # The phases of a level: the timed steps above record only the events a result needs (the level and the launches of k_select and
    # k_mstep -- gsr_hem_set_timing 1, the library's default: every event between two kernels is a packet of its own, 22 per level).
    # ONE more pass of the two clouds' levels, outside the timed region, with every phase event on, gives the breakdown.
    phase_pass = None
    if a.full and rank == 0 and a.mode == "replicas" and ctxs.get("serial"):
        m = ctxs["hem"]
        m.set_timing(2)
        m.set_rng("glibc", 1, 0)
        phase_pass = []
        for c in (src, tgt):
            phase_pass += hem_levels(m, c)[1]
        sync()
        m.set_timing(1)

    # measured device-copy bandwidth of this very GPU (SURVEY 8d asks for the fraction of both the nominal and a measured
    # figure): 1 GiB device-to-device, read + write traffic
    copy_gbs = None
    if a.full and rank == 0:
        try:
            src_t = torch.empty(1 << 28, dtype=torch.float32, device=dev)
            dst_t = torch.empty_like(src_t)
            dst_t.copy_(src_t); sync()
            tc = time.perf_counter()
            for _ in range(5):
                dst_t.copy_(src_t)
            sync()
            copy_gbs = 5 * 2.0 * src_t.numel() * 4 / (time.perf_counter() - tc) / 1e9
            del src_t, dst_t
        except Exception:
            copy_gbs = None

    strong = None
    if a.full and world > 1 and a.mode == "replicas" and not a.no_strong:
        # the replica measurement is complete: free its clouds, then the strong-scaling children (guarded: nothing that happens in
        # them can lose the line below)
        del src, tgt
        torch.cuda.empty_cache()
        strong = run_strong_children(a, rank, world, barrier)

    if rank == 0:
        F = 45
        last = runs[-1]
        kern = [k for r in runs for k in r["kern"]]
        phases = {p: sum(k[p] for k in kern) / a.steps for p in ("ms_level", "ms_k_select_count", "ms_k_select_fill", "ms_k_select", "ms_k_mstep")}
        if phase_pass:
            phases.update({p: sum(k[p] for k in phase_pass) for p in ("ms_grid", "ms_select", "ms_sumlw", "ms_mstep", "ms_flags", "ms_k_partition", "ms_k_bucket_sum")})
            phases["ms_level_with_every_phase_event"] = sum(k["ms_level"] for k in phase_pass)
            phases["note"] = ("ms_level and ms_k_* of the first line: the timed steps (events around the level, k_select and k_mstep only); the phases: one "
                              "extra untimed pass with all 22 events of a level on (ms_level_with_every_phase_event is that pass's total)")
        # the two big kernels, each timed by hipEvent pairs on the library's stream around every launch (gsr_hem_get_kernel_ms):
        # k_select (child selection + likelihood) and k_mstep (moment matching).  The roofline object prices the one with the larger
        # total time.  Algorithmic bytes of a launch = SURVEY 8(d)'s bytes_level of ITS level.
        lvl_b = np.array([bytes_level(k["n_in"], k["n_out"], F) for k in kern], dtype=np.float64)
        n_in = np.array([k["n_in"] for k in kern], dtype=np.float64)
        per_kernel = {}
        for kname, key in (("k_select", "ms_k_select"), ("k_mstep", "ms_k_mstep")):
            ms = np.array([k[key] for k in kern])
            per_kernel[kname] = {"total_ms_per_step": float(ms.sum() / a.steps), "avg_launch_ms": float(ms.mean()) if len(ms) else 0.0,
                                 "achieved_GBps": float(lvl_b.mean() / (ms.mean() * 1e-3) / 1e9) if len(ms) and ms.mean() > 0 else 0.0}
        dom = max(per_kernel, key=lambda k: per_kernel[k]["total_ms_per_step"])
        dom_key = {"k_select": "ms_k_select", "k_mstep": "ms_k_mstep"}[dom]
        sel_ms = np.array([k[dom_key] for k in kern])
        avg_ms = float(sel_ms.mean()) if len(sel_ms) else 0.0
        achieved = float(lvl_b.mean() / (avg_ms * 1e-3) / 1e9) if avg_ms > 0 else 0.0
        big_n = max(k["n_in"] for k in kern) if kern else n
        lvl1 = [k for k in kern if k["n_in"] == big_n]
        l1_bytes = float(np.mean([bytes_level(k["n_in"], k["n_out"], F) for k in lvl1])) if lvl1 else 0.0
        l1_ms = float(np.mean([k["ms_level"] for k in lvl1])) if lvl1 else 0.0
        l1_sel = float(np.mean([k["ms_k_select"] for k in lvl1])) if lvl1 else 0.0
        l1_mst = float(np.mean([k["ms_k_mstep"] for k in lvl1])) if lvl1 else 0.0
        desc = {"k_select": "k_select<SPARSE> (child selection + likelihood, one wavefront per parent)",
                "k_mstep": "k_mstep (responsibilities + moment matching: one 64-byte record and one 192-byte SH row gathered per pair)"}
        pmc, pmc_note = pmc_summary({"k_select": "gsr::k_select<2, 2, false>", "k_mstep": "gsr::k_mstep<4, 1, false>"}[dom])
        roof = {"bound": "hbm", "kernel": desc[dom],
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "bytes_model": "SURVEY 8(d) bytes_level = n_in (57 + 4F + 16) + n_out (57 + 4F) of the launch's level, / launch duration",
                "avg_launch_ms": avg_ms, "launches": int(len(sel_ms)), "avg_units_per_launch": float(n_in.mean()) if len(n_in) else 0.0,
                "avg_algorithmic_bytes_per_launch": float(lvl_b.mean()) if len(lvl_b) else 0.0,
                "traffic": None, "measured_copy_GBps": copy_gbs, "frac_of_measured_copy": (achieved / copy_gbs) if copy_gbs else None,
                "kernels": per_kernel,
                "level1": {"n_in": int(big_n), "algorithmic_bytes": l1_bytes, "ms_level": l1_ms, "ms_k_select": l1_sel, "ms_k_mstep": l1_mst,
                           "level_GBps": l1_bytes / (l1_ms * 1e-3) / 1e9 if l1_ms else None,
                           "level_frac": l1_bytes / (l1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if l1_ms else None,
                           "k_select_GBps": l1_bytes / (l1_sel * 1e-3) / 1e9 if l1_sel else None,
                           "k_select_frac": l1_bytes / (l1_sel * 1e-3) / 1e9 / HBM_PEAK_GBS if l1_sel else None,
                           "k_mstep_frac": l1_bytes / (l1_mst * 1e-3) / 1e9 / HBM_PEAK_GBS if l1_mst else None},
                "why_not_hbm_bound": "the level evaluates ~170 candidate tests and ~50 KL divergences per input splat and gathers 256 bytes per accepted pair "
                                     "(22 pairs per splat) -- neighbour work the 8(d) byte model does not count: k_select is bound by VALU issue and L2 request rate, "
                                     "k_mstep by the L2 -> CU gather rate (28 GB per 5 M level), see DESIGN.md 4"}
        lvl_pmc, _ = pmc_summary("level_total")
        if lvl_pmc and l1_bytes:
            # the whole 5 M level's HBM traffic (every gsr:: kernel of it, the same PMC passes) against SURVEY 8(d)'s algorithmic bytes
            roof["level1"].update({"traffic_raw": lvl_pmc["traffic_raw"], "traffic": lvl_pmc["traffic_x2"],
                                   "traffic_raw_over_algorithmic": lvl_pmc["traffic_raw"] / l1_bytes, "traffic_over_algorithmic": lvl_pmc["traffic_x2"] / l1_bytes,
                                   "traffic_source": lvl_pmc["source"] + " (level_total: FETCH_SIZE + WRITE_SIZE of every gsr:: kernel of one level; `traffic` with FETCH_SIZE x 2)"})
        if pmc:
            rd_raw, wr = pmc.get("hbm_read_bytes_per_launch_raw", 0.0), pmc.get("hbm_write_bytes_per_launch", 0.0)
            roof["traffic"] = pmc.get("hbm_read_bytes_per_launch_x2_corrected", 0.0) + wr
            roof["traffic_source"] = pmc["source"] + " (level-1 launch at 5 M; FETCH_SIZE x2 per MI355X_MICROARCH.md)"
            # MI355X_MICROARCH.md: "other access widths are uncalibrated: calibrate on a known byte count in your own access pattern".
            # profiles/archive/r03_fetch_calibration.txt: FETCH_SIZE counts streams at x0.5 but random 64-byte records in full -- the x2 doubles
            # the gathers of these two kernels.  Calibrated: raw + the half of the kernel's STREAMED bytes the counter leaves out
            # (k_mstep: the pair list, 8 B per pair, and the 32-byte headers; k_select: nothing of size is streamed from HBM).
            lv1 = [k for k in kern if k["n_in"] == big_n]
            streamed = float(np.mean([8.0 * k["pairs"] + 32.0 * k["parents"] for k in lv1])) if (dom == "k_mstep" and lv1) else 0.0
            roof["traffic_raw"] = rd_raw + wr
            roof["traffic_calibrated"] = rd_raw + 0.5 * streamed + wr
            roof["traffic_note"] = ("traffic = FETCH_SIZE x 2 + WRITE_SIZE (the guide's streaming-read correction, kept for comparison with "
                                    "earlier rounds); traffic_calibrated = FETCH_SIZE + half of the kernel's streamed bytes + WRITE_SIZE "
                                    "(profiles/archive/r03_fetch_calibration.txt: gathers of 64-byte records are counted in full)")
            vi, va = pmc.get("SQ_INSTS_VALU_per_launch"), pmc.get("SQ_ACTIVE_INST_VALU_per_launch")
            busy = pmc.get("SQ_BUSY_CYCLES_per_launch")
            roof["valu"] = {"insts_per_launch": vi, "active_quad_cycles_per_launch": va,
                            "measured_cycles_per_inst": (4.0 * va / vi) if vi and va else None,
                            "valu_busy_frac": (4.0 * va / 1024.0) / (busy / 32.0) if va and busy else None,
                            "issue_cost_cycles_microbench": VALU_CYCLES, "source": pmc["source"]}
        else:
            roof["traffic_note"] = pmc_note
            roof["valu"] = {"issue_cost_cycles_microbench": VALU_CYCLES, "note": pmc_note}
        fin = last["levels"][-1]
        per_eval = fin["ms_iters"] / max(1, fin["evals"])
        roof["icp_finest"] = {"ns": fin["ns"], "nt": fin["nt"], "ms_per_iteration": per_eval, "iterations_per_sec": 1e3 / per_eval if per_eval else None,
                              "algorithmic_bytes_per_iteration": 36.0 * fin["ns"],
                              "achieved_GBps": 36.0 * fin["ns"] / (per_eval * 1e-3) / 1e9 if per_eval else None,
                              "frac": 36.0 * fin["ns"] / (per_eval * 1e-3) / 1e9 / HBM_PEAK_GBS if per_eval else None}
        coarse = last["levels"][0]
        gpu_icp_coarse = coarse["evals"] / (coarse["ms_iters"] * 1e-3) if coarse["ms_iters"] else None
        par = {"replicas": f"{world} independent pair(s), one per GPU, no data-path collective",
               "c4": f"cloud A HEM on rank 0, cloud B on rank 1, levels broadcast once, ICP source split over {world} ranks + all-reduce of 32 doubles per iteration",
               "c5": f"source cloud spatially partitioned over {world} rank(s): halo rows + integer partial sums per HEM level through the library's "
                     f"communicator ({comm.transport if comm else 'none'}), levels stay distributed; target levels replicated; ICP shard = the rank's piece, "
                     "one all-reduce of 32 float64 per iteration"}[a.mode]
        line = {
            "metric": "Gaussians/sec through HEM level + ICP iters/sec, 2x5M-splat pair",
            "value": hem_gauss / hem_s,
            "unit": "Gaussians/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3,
            "higher_is_better": True, "scaling": "weak" if a.mode == "replicas" else "strong", "vs_baseline": None,
            "dtype": "f32 (HEM) / f64 (ICP)", "data": "synthetic",
            "config": {"workload": (f"2x{n} synthetic splats (SH deg 3{', surfel shapes' if a.workload == 'aniso' else (', clustered scene' if a.workload == 'clustered' else '')}) per GPU: 3 HEM levels per cloud + "
                                    "4-level coarse-to-fine point-to-plane ICP (BASELINE configs[2])") if a.mode == "replicas" else
                                   (f"2x{n} splats, clouds one per GPU + ICP source split (BASELINE configs[3])" if a.mode == "c4" else
                                    f"one {n}-splat cloud vs a {min(a.target_splats, n)}-splat target, sharded HEM + split ICP (BASELINE configs[4])"),
                       "mode": a.mode, "splat_shapes": a.workload, "pair": {"angle_deg": PAIR_ANGLE_DEG, "shift_h": PAIR_SHIFT_H}, "hem_params": HEM_PARAMS, "iter_values": ITER_VALUES, "max_corr": MAX_CORR, "level_sizes": last["level_sizes"],
                       "clouds": (("serial: cloud 1 then cloud 2 on one context and ONE shared rand() stream (a single reference process); each cloud's three levels are one library call "
                                   "(gsr_hem_run_levels); the target's normals leave with its levels (side stream, inside the HEM phase); index builds and source sorts inside the ICP phase"
                                   if ctxs.get("serial") else
                                   "concurrent: the two clouds' HEM levels side by side on two contexts / streams (each cloud = a fresh reference process: rand() "
                                   "stream at position 0), every target level's normals computed by the target cloud's thread inside the HEM phase")
                                  if a.mode == "replicas" else "n/a"),
                       "parallelism": par},
            "icp_iters_per_sec": icp_iters / icp_s,
            "icp_iterations_per_step": last["icp_iters"],
            "icp_per_level": [{"ns": l["ns"], "iterations": l["iterations"], "ms_per_iteration": l["ms_iters"] / max(1, l["evals"]),
                               "ms_target_index_build": l["ms_build"]} for l in last["levels"]],
            "icp_note": "the pair is SURVEY 8(d)'s: 5 degrees about (1,1,1)/sqrt(3) and 0.05 h (1,-1,0.5) apart; the coarsest level uses its whole "
                        "budget of 50 iterations.  The blended icp_iters_per_sec is dominated by the coarse levels (~45 us per iteration at 185 k points: "
                        "a latency-bound grid walk per source point); the finest level's rate is roofline.icp_finest",
            "hem_s_per_step": hem_s / a.steps, "icp_s_per_step": icp_s / a.steps,
            "icp_result": {"fitness": last["fitness"], "inlier_rmse": last["rmse"], "T_err_vs_ground_truth_F": float(np.linalg.norm(last["T"] - T_gt))},
            "hem_phase_ms_per_step": phases,
            # per level of the LAST step, in order (cloud 1: levels 1-3, cloud 2: levels 1-3): input size, time, host round trips (1 = the asynchronous
            # schedule: one answer behind the level's last kernel), schedule (1 asynchronous, 0 synchronous, 2 an asynchronous attempt rerun)
            "hem_levels_last_step": [{"n_in": k["n_in"], "n_out": k["n_out"], "ms_level": k["ms_level"], "round_trips": k.get("round_trips"),
                                      "schedule": k.get("schedule"), "dropped": k["dropped"]} for k in last["kern"]],
            "roofline": roof,
        }
        if a.mode == "c5":
            line["config"]["c5_scaling"] = c5_scaling
        if strong is not None:
            line["strong"] = strong
        if comm is not None:
            line["transport"] = comm.transport
        if "exchange_s" in last:
            line["exchange_s_per_step"] = sum(r["exchange_s"] for r in runs) / a.steps
        if "part" in last:
            line["partition_rank0"] = last["part"]
        if a.full and world == 1 and a.mode == "replicas" and a.workload == "iso":
            # ONE local registration on the full clouds (the LocalRegistrator path, qt_local_registrator.py:26-32: do_icp_registration(pc1, pc2, init,
            # params) with LocalRegistrationParams' defaults, registration_parameters.py:7-15 -- point-to-point, 30 iterations, 1e-6 / 1e-6) from a start
            # 0.5 degrees and 0.5 max_corr off the answer: the fine-level search kernel over its whole budget instead of the two iterations the
            # coarse-to-fine schedule leaves it.  max_correspondence = the schedule's finest (the default, 5.0 scene units, is
            # the whole scene).  Outside the timed region.
            try:
                from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
                est0 = lru.get_estimation(lru.LocalRegistrationType.ICP_Point_To_Point, lru.RobustLoss(0))
                off = synth.rigid_transform(0.5, (0.3, -1.0, 0.5), 0.5 * MAX_CORR[-1] * np.array([0.6, 0.5, -0.62]))
                s0, t0 = PointCloud(xyz32=src["xyz"]), PointCloud(xyz32=tgt["xyz"])
                best = None
                for _ in range(2):
                    sync(); tw = time.perf_counter()
                    r1 = lru.registration_icp(s0, t0, MAX_CORR[-1], off @ T_gt, est0, lru.get_convergence_criteria(1e-6, 1e-6, 30), device=device, ctx=ctxs["icp"])
                    sync(); tw = time.perf_counter() - tw
                    best = tw if best is None else min(best, tw)
                per = r1.timing["ms_iters"] / max(1, r1.timing["iter_kernels"])
                line["icp_single_level_5m"] = {"workload": f"registration_icp on the {n} x {n} level-0 clouds, point-to-point, max_corr {MAX_CORR[-1]}, <= 30 iterations, start 0.5 degrees / "
                                                           f"{0.5 * MAX_CORR[-1]:.3f} off the ground truth", "iterations": r1.iterations, "evaluations": r1.timing["iter_kernels"],
                                               "ms_total": best * 1e3, "ms_target_index_build": r1.timing["ms_build"], "ms_iterations": r1.timing["ms_iters"], "ms_per_iteration": per,
                                               "algorithmic_bytes_per_iteration": 24.0 * n, "achieved_GBps": 24.0 * n / (per * 1e-3) / 1e9 if per else None,
                                               "frac_of_hbm_peak": 24.0 * n / (per * 1e-3) / 1e9 / HBM_PEAK_GBS if per else None,
                                               "fitness": r1.fitness, "inlier_rmse": r1.inlier_rmse, "T_err_vs_ground_truth_F": float(np.linalg.norm(r1.transformation - T_gt))}
            except Exception as e:  # pragma: no cover
                line["icp_single_level_5m"] = {"error": str(e)[:200]}
        if a.full and world == 1 and a.mode == "replicas" and a.workload == "iso" and not a.no_aniso:
            # the same level on the surfel workload (real 3DGS splats are flat discs and needles, far outside the condition numbers of the
            # isotropic recipe): one 5 M-splat cloud, level 1, beside the isotropic level above
            try:
                ca = synth.make_cloud_torch(n, seed=300, device=dev, shape="aniso")
                m = ctxs["hem"]
                rows = []
                for _ in range(5):                  # (the first repetitions on another shape grow the context's buffers: the last three count)
                    m.set_rng("glibc", 1, 0)
                    m.set_level0(ca["xyz"], ca["color"], ca["opacity"], ca["cov6"], ca["sh"], borrow=True)
                    m.run_level()
                    rows.append(m.stats())
                st = rows[-1]
                ms = float(np.median([r["ms_level"] for r in rows[2:]]))
                c6 = ca["cov6"][:200000].double().cpu().numpy()
                ev = np.linalg.eigvalsh(np.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], 1))
                line["aniso_level"] = {"workload": f"one {n}-splat cloud, synth shape 'aniso' (60 % discs, 15 % needles on a smooth orientation field), level 1",
                                       "condition_number_percentiles_50_90_99": [float(v) for v in np.percentile(ev[:, 2] / ev[:, 0], [50, 90, 99])],
                                       "irregular_fraction": st["irregular"] / st["n_in"], "parents": st["parents"],
                                       "candidates_per_parent": st["candidates"] / max(1, st["parents"]), "pairs": st["pairs"], "orphans": st["orphans"],
                                       "n_out": st["n_out"], "dropped": st["dropped"], "round_trips": st["round_trips"], "schedule": st["schedule"],
                                       "ms_level": ms, "ms_k_select": st["ms_k_select"], "ms_k_mstep": st["ms_k_mstep"],
                                       "gaussians_per_s": st["n_in"] / (ms * 1e-3),
                                       "iso_level1_ms_same_n": l1_ms, "ratio_to_iso_level": ms / l1_ms if l1_ms else None}
                del ca
            except Exception as e:  # pragma: no cover
                line["aniso_level"] = {"error": str(e)[:200]}
            # and on the large-scene shape the reference's README complains about (README.md:113): dense clumps on a sparse background,
            # a handful of giant splats, far outliers -- heavy parents, long grid rows, crowded sum buckets.  No silent fallback: the
            # overflow / two-pass flags of the level ride along.
            try:
                cc = synth.make_cloud_torch(n, seed=400, device=dev, shape="clustered")
                m = ctxs["hem"]
                rows = []
                for rep in range(6):
                    m.set_timing(2 if rep == 5 else 1)                  # two to grow the buffers, three timed like the isotropic level, a sixth with the phase events on
                    m.set_rng("glibc", 1, 0)
                    m.set_level0(cc["xyz"], cc["color"], cc["opacity"], cc["cov6"], cc["sh"], borrow=True)
                    m.run_level()
                    rows.append(m.stats())
                m.set_timing(1)
                st = rows[-1]
                ms = float(np.median([r["ms_level"] for r in rows[2:5]]))
                line["clustered_level"] = {"workload": f"one {n}-splat cloud, synth shape 'clustered' (60 % in 40 Gaussian clumps of 30-100 x the background density with "
                                                       "splats shrunk by the cube root of that, 6 giants of 40 x sigma, 12 outliers at 20-60 h), level 1",
                                           "parents": st["parents"], "candidates_per_parent": st["candidates"] / max(1, st["parents"]), "pairs": st["pairs"],
                                           "orphans": st["orphans"], "n_out": st["n_out"], "cells": st["cells"], "irregular_fraction": st["irregular"] / st["n_in"],
                                           "heavy_parents": st["heavy_parents"], "heavy_work_items": st["heavy_work_items"],
                                           "one_pass_selection": bool(st["one_pass"]), "bucket_region_overflow_fallback": bool(st["partition_overflow"]),
                                           "ms_level": ms, "ms_phases": {k: st[k] for k in ("ms_grid", "ms_select", "ms_sumlw", "ms_mstep", "ms_flags")},
                                           "ms_k_select": st["ms_k_select"], "ms_k_mstep": st["ms_k_mstep"], "gaussians_per_s": st["n_in"] / (ms * 1e-3),
                                           "iso_level1_ms_same_n": l1_ms, "ratio_to_iso_level": ms / l1_ms if l1_ms else None}
                del cc
                ctxs["hem"].close()                                     # (a context that overflowed stays with the exact partition: a fresh one for what follows)
                ctxs["hem"] = hem.HemMixture(device=device, rng_mode="glibc", **HEM_PARAMS)
            except Exception as e:  # pragma: no cover
                line["clustered_level"] = {"error": str(e)[:200]}
        if a.full and world == 1 and a.mode == "replicas" and not a.no_cpu_baseline:
            def gpu_level1_rate(nn):
                c = synth.make_cloud(nn, seed=0)
                dc = {k: torch.from_numpy(v).to(dev) for k, v in c.items() if isinstance(v, np.ndarray)}
                m = ctxs["hem"]
                best = None
                for _ in range(3):
                    m.set_rng("glibc", 1, 0)
                    m.set_level0(dc["xyz"], dc["color"], dc["opacity"], dc["cov6"], dc["sh"])
                    sync(); t = time.perf_counter()
                    m.run_level()
                    sync(); dt = time.perf_counter() - t
                    best = dt if best is None else min(best, dt)
                return nn / best
            line["cpu_baseline"] = cpu_baseline(gpu_level1_rate, gpu_icp_coarse)
        print(json.dumps(line), flush=True)
    barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
