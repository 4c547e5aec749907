"""Mixture-to-mixture registration on the MI355X, measured: writes profiles/d2d_bench.json.

    python scripts/bench_d2d.py [--n 1000000] [--radii 0.1 0.2] [--repeats 7] [--out profiles/d2d_bench.json]

The benchmark's pair at n splats a side (a cloud and its copy moved by 5 degrees / 0.05 h with 0.002 position noise, SH degree 0), at
the transform a Generalized ICP of the pair converges to.  Per radius, alternating in one run: the device time of one
gsr_icp_accumulate Generalized-ICP evaluation of the pair (the yardstick: same metric, one nearest match per row, a kernel this feature
does not touch) and of one gsr_d2d_accumulate, by events on the stream around each call (the read-back of the sums included, for both
alike).  Medians, the spread over the repeats, the ratio, and the mean number of pairs per source row, which is what the cost scales
with.  Then one whole gsr_d2d_register from the ground truth at the first radius: wall time and iterations.  No target is fixed:
nobody had measured any of this.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIR_ANGLE_DEG, PAIR_SHIFT_H = 5.0, 0.05


def stat(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / statistics.median(v)}


def pair(n):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import synth
    dev = "cuda:0"
    tgt = synth.make_cloud_torch(n, seed=1, device=dev, sh_degree=0)
    T_gt = synth.rigid_transform(PAIR_ANGLE_DEG, (1, 1, 1), PAIR_SHIFT_H * tgt["h"] * np.array([1.0, -1.0, 0.5]))
    src = synth.apply_rigid_torch(tgt, np.linalg.inv(T_gt))
    gen = torch.Generator(device=dev).manual_seed(7)
    sx = (src["xyz"] + torch.randn(src["xyz"].shape, device=dev, generator=gen) * 0.002).contiguous()
    return tgt, src, sx, T_gt


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    res = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--radii", type=float, nargs="+", default=[0.1, 0.2])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d2d_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import d2d, icp
    tgt, src, sx, T_gt = pair(a.n)
    tx, tc, sc = tgt["xyz"].contiguous(), tgt["cov6"].contiguous(), src["cov6"].contiguous()
    stream = torch.cuda.current_stream(0)
    res = {"device": torch.cuda.get_device_name(0), "n_source": a.n, "n_target": a.n, "repeats": a.repeats, "radii": [],
           "note": f"device times by events on the stream, medians of {a.repeats} alternating repeats after 2 warm-up rounds; spread = (max - min) / median"}
    with icp.IcpContext(device=0) as ctx, d2d.D2DContext(0) as dctx:
        T = None
        for radius in a.radii:
            ctx.set_target(tx, None, radius)
            ctx.set_source(sx)
            ctx.set_target_cov(tc)
            ctx.set_source_cov(sc)
            if T is None:
                r = ctx.register(T_gt, kind=icp.KIND_GENERALIZED, max_iter=30)
                T = r["transformation"]
                res.update(gicp_fitness=r["fitness"], gicp_inlier_rmse=r["inlier_rmse"], T_error=float(np.linalg.norm(T - T_gt)))
            dctx.set_target(tx, tc, None, radius)
            dctx.set_source(sx, sc, None)
            for _ in range(2):                               # warm-up: code objects, workspaces
                ctx.accumulate(T, icp.KIND_GENERALIZED)
                dctx.accumulate(T)
            ev, da = [], []
            for _ in range(a.repeats):
                ms, acc = timed(stream, lambda: ctx.accumulate(T, icp.KIND_GENERALIZED))
                ev.append(ms)
                ms, sums = timed(stream, lambda: dctx.accumulate(T))
                da.append(ms)
            row = {"max_corr": radius, "icp_evaluation_generalized": stat(ev), "d2d_accumulate": stat(da), "n_pairs": int(sums[29]),
                   "mean_pairs_per_source_row": float(sums[29]) / a.n, "rows_with_pairs": int(sums[30]), "n_singular": int(sums[31]), "score": float(sums[27]),
                   "n_correspondences_icp": int(acc[0]), "ratio_d2d_over_evaluation": statistics.median(da) / statistics.median(ev),
                   "ns_per_pair": 1e6 * statistics.median(da) / max(float(sums[29]), 1.0)}
            res["radii"].append(row)
            print(json.dumps(row), flush=True)
        dctx.set_target(tx, tc, None, a.radii[0])
        dctx.set_source(sx, sc, None)
        dctx.register(T_gt, max_iteration=2)                 # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = dctx.register(T_gt)
        wall = time.perf_counter() - t0
        res["registration"] = {"max_corr": a.radii[0], "wall_s": wall, "iterations": r["iterations"], "status": r["status"], "score": r["score"],
                               "fitness": r["fitness"], "T_error": float(np.linalg.norm(r["transformation"] - T_gt))}
        print(json.dumps(res["registration"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
