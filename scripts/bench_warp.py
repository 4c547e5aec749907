"""Non-rigid refinement on the MI355X, measured: writes profiles/warp_bench.json.

    python scripts/bench_warp.py [--sizes 1000000 5000000] [--repeats 7] [--out profiles/warp_bench.json]

(a) Per size n and lattice (5^3, 9^3): the benchmark's pair (a cloud and its copy moved by 5 degrees / 0.05 h with 0.002 position noise,
SH degree 0), registered by point-to-plane ICP at the finest correspondence distance (0.1); the source moved by the result is the
warp context's source.  Alternating in one run: the device time of one gsr_icp_accumulate point-to-plane evaluation of the same pair
(the yardstick: a kernel this feature does not touch) and of one gsr_warp_accumulate at U = 0, by events on the stream around each call
(the read-back of the sums included, for both alike).  Medians, the spread over the repeats and the ratio.
(b) gsr_model_warp of the largest size's splats against gsr_model_transform of the same arrays (positions and covariances; SH degree 0).
(c) The host solve (gsr_warp_solve) at 5^3 and 9^3 on the sums of (a): wall time.
(d) A whole default refinement (3 levels, 6 iterations each) of the smallest size's pair: wall time and its split.
No ratio is fixed: nobody had measured any of this.
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
MAX_CORR = 0.1
PAIR_ANGLE_DEG, PAIR_SHIFT_H = 5.0, 0.05


def stat(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / statistics.median(v)}


def pair(n):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import icp, synth
    dev = "cuda:0"
    tgt = synth.make_cloud_torch(n, seed=1, device=dev, sh_degree=0)
    T_gt = synth.rigid_transform(PAIR_ANGLE_DEG, (1, 1, 1), PAIR_SHIFT_H * tgt["h"] * np.array([1.0, -1.0, 0.5]))
    src = synth.apply_rigid_torch(tgt, np.linalg.inv(T_gt))
    gen = torch.Generator(device=dev).manual_seed(7)
    sx = (src["xyz"] + torch.randn(src["xyz"].shape, device=dev, generator=gen) * 0.002).contiguous()
    return tgt, src, sx, icp.normals_from_cov(tgt["cov6"], device=0), T_gt


def timed(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    res = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), res


def accumulate_times(n, repeats, keep_sums):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import icp, warp
    tgt, src, sx, normals, T_gt = pair(n)
    stream = torch.cuda.current_stream(0)
    out = {"n_source": n, "n_target": n, "max_corr": MAX_CORR, "lattices": {}}
    with icp.IcpContext(device=0) as ctx, warp.WarpContext(0) as wctx:
        ctx.set_target(tgt["xyz"].contiguous(), normals, MAX_CORR)
        ctx.set_source(sx)
        r = ctx.register(T_gt, kind=icp.KIND_POINT_TO_PLANE, max_iter=30)
        T = r["transformation"]
        out.update(fitness=r["fitness"], inlier_rmse=r["inlier_rmse"], T_error=float(np.linalg.norm(T - T_gt)))
        moved = warp._moved_f32(sx, T)
        wctx.set_target(tgt["xyz"].contiguous(), normals, MAX_CORR)
        wctx.set_source(moved)
        lo, hi = warp.default_box(moved.cpu().numpy())
        for nodes in (5, 9):
            fld = warp.WarpField(warp.WarpLattice(lo, hi, (nodes,) * 3))
            for _ in range(2):                               # warm-up: code objects, workspaces
                ctx.accumulate(T, icp.KIND_POINT_TO_PLANE)
                wctx.accumulate(fld)
            ev, wa = [], []
            for _ in range(repeats):
                ms, acc = timed(stream, lambda: ctx.accumulate(T, icp.KIND_POINT_TO_PLANE))
                ev.append(ms)
                ms, (sums, n_corr, rmse) = timed(stream, lambda: wctx.accumulate(fld))
                wa.append(ms)
            keep_sums[nodes] = sums
            out["lattices"][f"{nodes}^3"] = {"icp_evaluation_point_to_plane": stat(ev), "warp_accumulate": stat(wa), "n_correspondences": n_corr,
                                             "n_correspondences_icp": int(acc[0]), "rmse": rmse, "cells_with_data": int((sums[:, 325] > 0).sum()),
                                             "ratio_warp_over_evaluation": statistics.median(wa) / statistics.median(ev)}
    return out


def model_times(n, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import synth, warp
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    c = synth.make_cloud_torch(n, seed=2, device="cuda:0", sh_degree=0)
    g = GaussianModel("cuda:0").from_arrays(c["xyz"], c["color"], c["opacity"], c["cov6"], c["sh"], 0)
    T = synth.rigid_transform(PAIR_ANGLE_DEG, (1, 1, 1), (0.1, -0.1, 0.05))
    lo, hi = warp.default_box(c["xyz"].cpu().numpy())
    fld = warp.WarpField(warp.WarpLattice(lo, hi, (5, 5, 5)), 0.01 * c["h"] * np.random.default_rng(0).normal(size=(125, 3)))
    stream = torch.cuda.current_stream(0)
    for _ in range(2):
        g._transform_kernel(T, False)
        fld.apply_arrays(g._xyz, g._covariance)
    tr, wp = [], []
    for _ in range(repeats):
        tr.append(timed(stream, lambda: g._transform_kernel(T, False))[0])
        ms, (_, _, folded) = timed(stream, lambda: fld.apply_arrays(g._xyz, g._covariance))
        wp.append(ms)
    return {"n": n, "model_transform": stat(tr), "model_warp": stat(wp), "n_folded": folded, "ratio_warp_over_transform": statistics.median(wp) / statistics.median(tr)}


def solve_times(sums_by_nodes, repeats):
    from gaussiansplattingregistration_amd import warp
    out = {}
    for nodes, sums in sums_by_nodes.items():
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            _, rep = warp.solve((nodes,) * 3, sums, 0.01, 1e-6)
            ms.append((time.perf_counter() - t0) * 1e3)
        out[f"{nodes}^3"] = dict(stat(ms), n_unknowns=rep["n_unknowns"], half_band=rep["half_band"])
    return out


def refinement(n):
    import torch
    from gaussiansplattingregistration_amd import warp
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.params import WarpParams
    tgt, src, sx, normals, T_gt = pair(n)
    run = lambda: warp.NonRigidRefiner(PointCloud(xyz32=sx), PointCloud(xyz32=tgt["xyz"].contiguous(), normals=normals), WarpParams(max_corr=MAX_CORR), init=T_gt).run()
    run()                                                    # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = run()
    wall = time.perf_counter() - t0
    return {"n": n, "wall_s": wall, "timings_s": r.timings, "rmse_before": r.rmse_before, "rmse_after": r.rmse_after, "n_corr": r.n_corr,
            "solves": sum(len(lv["iterations"]) for lv in r.levels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 5000000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "accumulate": [], "note": "device times by events on the stream, medians of "
           f"{a.repeats} alternating repeats after 2 warm-up rounds; spread = (max - min) / median"}
    sums = {}
    for n in a.sizes:
        sums = {}
        res["accumulate"].append(accumulate_times(n, a.repeats, sums))
        print(json.dumps(res["accumulate"][-1]), flush=True)
    res["model"] = model_times(max(a.sizes), a.repeats)
    print(json.dumps(res["model"]), flush=True)
    res["solve"] = solve_times(sums, a.repeats)
    print(json.dumps(res["solve"]), flush=True)
    res["refinement"] = refinement(min(a.sizes))
    print(json.dumps(res["refinement"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
