"""Multiway registration on the MI355X, measured: writes profiles/multiway_bench.json.

    python scripts/bench_multiway.py [--sizes 1000000 5000000] [--repeats 7] [--fragment 1000000] [--out profiles/multiway_bench.json]

(a) Per size n: the benchmark's pair (a cloud and its copy moved by 5 degrees / 0.05 h with 0.002 position noise, SH degree 0), one
context at the finest correspondence distance (0.1) with the target's covariance normals, point-to-plane ICP from the known
transform to convergence, and there -- alternating in one run -- the device time of one gsr_icp_accumulate point-to-plane evaluation
(the yardstick: an entry this measurement does not touch) and of one gsr_icp_information call, by events on the context's stream
around each call (the read-back of the sums included, for both alike).  Medians, the spread (min, max) over the repeats, and the
ratio information / evaluation.  Expectation: the ratio is at most 1.10 -- the same search with a third of the accumulators.
(b) Wall time of a 4-scene multiway run on four slabs of `--fragment` splats cut from one cloud (neighbours share a third of the
width, as in tests/test_multiway_gpu.py), split into pairwise registration, information matrices, optimisation and merge.  No target.
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


def kernel_times(n, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import icp, synth
    dev = "cuda:0"
    tgt = synth.make_cloud_torch(n, seed=1, device=dev, sh_degree=0)
    T_gt = synth.rigid_transform(PAIR_ANGLE_DEG, (1, 1, 1), PAIR_SHIFT_H * tgt["h"] * np.array([1.0, -1.0, 0.5]))
    src = synth.apply_rigid_torch(tgt, np.linalg.inv(T_gt))
    gen = torch.Generator(device=dev).manual_seed(7)
    sx = (src["xyz"] + torch.randn(src["xyz"].shape, device=dev, generator=gen) * 0.002).contiguous()
    normals = icp.normals_from_cov(tgt["cov6"], device=0)
    out = {"n_source": n, "n_target": n, "max_corr": MAX_CORR}
    with icp.IcpContext(device=0) as ctx:
        ctx.set_target(tgt["xyz"].contiguous(), normals, MAX_CORR)
        ctx.set_source(sx)
        r = ctx.register(T_gt, kind=icp.KIND_POINT_TO_PLANE, max_iter=30)
        T = r["transformation"]
        out.update(fitness=r["fitness"], inlier_rmse=r["inlier_rmse"], iterations=r["iterations"], T_error=float(np.linalg.norm(T - T_gt)))
        stream = torch.cuda.current_stream(0)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            res = fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1), res
        for _ in range(2):                                   # warm-up: code objects, workspaces
            ctx.accumulate(T, icp.KIND_POINT_TO_PLANE)
            ctx.information(T)
        ev, inf = [], []
        for _ in range(repeats):
            ms, acc = timed(lambda: ctx.accumulate(T, icp.KIND_POINT_TO_PLANE))
            ev.append(ms)
            ms, (info, n_corr) = timed(lambda: ctx.information(T))
            inf.append(ms)
        assert n_corr == int(acc[0]), (n_corr, acc[0])        # the two calls ran the same search
    stat = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    out["evaluation_point_to_plane"] = stat(ev)
    out["information"] = stat(inf)
    out["n_correspondences"] = n_corr
    out["ratio_information_over_evaluation"] = statistics.median(inf) / statistics.median(ev)
    out["spread_evaluation"] = (max(ev) - min(ev)) / statistics.median(ev)
    out["spread_information"] = (max(inf) - min(inf)) / statistics.median(inf)
    return out


def multiway(fragment):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.params.registration_parameters import LocalRegistrationParams
    from gaussiansplattingregistration_amd.utils.local_registration_util import LocalRegistrationType
    from gaussiansplattingregistration_amd.workers.multiway import MultiwayRegistrator
    dev = "cuda:0"
    cloud = synth.make_cloud_torch(2 * fragment, seed=2, device=dev, sh_degree=0)
    h = cloud["h"]
    u = (cloud["xyz"][:, 0] + h) / (2 * h)
    rng = np.random.default_rng(42)
    edges = [(0, 1), (1, 2), (2, 3), (0, 2), (1, 3)]
    poses, models, clouds = [], [], []
    for i in range(4):
        sel = torch.nonzero((u >= i / 6) & (u <= i / 6 + 0.5)).reshape(-1)
        P = np.eye(4) if i == 0 else synth.rigid_transform(float(rng.uniform(5, 15)), rng.normal(size=3), rng.normal(size=3) * 0.2)
        sub = {k: cloud[k][sel].contiguous() for k in ("xyz", "color", "opacity", "cov6", "sh")}
        sub = synth.apply_rigid_torch(sub, np.linalg.inv(P))
        m = GaussianModel(dev).from_arrays(sub["xyz"], sub["color"], sub["opacity"], sub["cov6"], sub["sh"], 0)
        m._scaling = m._rotation = torch.empty(0, device=dev)
        poses.append(P)
        models.append(m)
        clouds.append(PointCloud(xyz32=m._xyz))
    gt = lambda s, t: np.linalg.inv(poses[t]) @ poses[s]
    init = {(s, t): synth.rigid_transform(0.5, rng.normal(size=3), rng.normal(size=3) * 0.006) @ gt(s, t) for s, t in edges}
    params = LocalRegistrationParams(registration_type=LocalRegistrationType.ICP_Point_To_Point, max_correspondence=0.05, max_iteration=30)
    out = {"fragment_sizes": [len(m) for m in models], "edges": edges, "max_corr": 0.05}
    for attempt in ("warm_up", "timed"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        worker = MultiwayRegistrator(clouds, params, edges=edges, init=init)
        res = worker.run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if res is None:
            raise SystemExit("multiway run failed: " + "; ".join(worker.errors))
        merged = GaussianModel.get_merged_gaussian_point_clouds_multi(models, res.poses)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        n_merged = len(merged)
        del merged
    out.update(pairwise_s=worker.timing["pairwise_s"], information_s=worker.timing["information_s"], optimization_s=worker.timing["optimization_s"],
               merge_s=t2 - t1, total_s=t2 - t0, merged_rows=n_merged,
               fitness=[r["fitness"] for r in res.edge_reports], icp_iterations=[r["iterations"] for r in res.edge_reports],
               n_correspondences=[r["n_correspondences"] for r in res.edge_reports], line_process=[r["line_process"] for r in res.edge_reports],
               pairwise_error=[float(np.linalg.norm(r["transformation"] - gt(r["source"], r["target"]))) for r in res.edge_reports],
               pose_error=[float(np.linalg.norm(X - P)) for X, P in zip(res.poses, poses)],
               optimizer_iterations=list(res.optimization.iterations), n_pruned=res.optimization.n_pruned)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fragment", type=int, default=1_000_000, help="splats per fragment of the 4-scene run (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiway_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    import torch
    doc = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "information_kernel": []}
    for n in a.sizes:
        r = kernel_times(n, a.repeats)
        print(json.dumps(r), flush=True)
        doc["information_kernel"].append(r)
        torch.cuda.empty_cache()
    if a.fragment:
        doc["four_scenes"] = multiway(a.fragment)
        print(json.dumps(doc["four_scenes"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
