"""Fast Global Registration on the MI355X: one JSON line with the time of each stage behind do_fgr_registration at the test scene's
size (about 4 k points per cloud) and at about 100 k points per cloud, beside the RANSAC stage of scripts/bench_global.py run in the
same process on the same clouds' sizes.

    python scripts/bench_fgr.py [--repeats 7] [--ransac-iters 100000] [--no-ransac]

Stages, on device-resident inputs, after a warm-up call each: matching (exact 1-NN both ways, the reciprocal pairs), the tuple test
(the scene as it is, and with tuple_scale = 1 where no triple can pass so that all 100 m trials run), the optimisation over the tuple
list and over the whole reciprocal set (64 iterations), the evaluation, and their total.  Every figure is the median over the
repeats of (a) the wall clock around the library call, which ends in the call's own stream wait, and (b) the time between two device
events recorded on the stream around it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _ms(fn, repeats):
    """-> ({"wall": median ms, "device": median ms}, last result) after one warm-up call"""
    import torch
    out = fn()
    wall, dev = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return {"wall": statistics.median(wall), "device": statistics.median(dev)}, out


def run(n_splats, voxel, repeats):
    import torch
    import global_model as G
    from gaussiansplattingregistration_amd import features as F
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    T = G.make_T()
    a, b = G.make_scene(n_splats, 1), G.transform_scene(G.make_scene(n_splats, 2), T)
    clouds = []
    for sc in (a, b):
        d = PointCloud(xyz32=torch.from_numpy(sc["xyz"]).cuda(), cov6=torch.from_numpy(sc["cov6"]).cuda()).voxel_down_sample(voxel)
        d.estimate_normals()
        clouds.append(U.orient_normals_towards_centroid(d))
    da, db = clouds
    prm = U.KDTreeSearchParamHybrid(5 * voxel, 100)
    fa, fb = U.compute_fpfh_feature(da, prm), U.compute_fpfh_feature(db, prm)
    mc = 1.5 * voxel
    ms_match, (corres, _) = _ms(lambda: F.feature_match(fa.rows, fb.rows, mutual=True, ransac_n=0), repeats)
    m = int(corres.shape[0])
    ms_tuple, (tuples, n_trials) = _ms(lambda: F.fgr_tuple_test(da.xyz32, db.xyz32, corres, 0.95, 1000), repeats)
    ms_tuple_all, (none, n_all) = _ms(lambda: F.fgr_tuple_test(da.xyz32, db.xyz32, corres, 1.0, 1000), repeats)
    assert int(none.shape[0]) == 0 and n_all == 100 * m
    ms_opt, r = _ms(lambda: F.fgr_optimize(da.xyz32, db.xyz32, tuples, maximum_correspondence_distance=mc), repeats)
    ms_opt_full, rf = _ms(lambda: F.fgr_optimize(da.xyz32, db.xyz32, corres, maximum_correspondence_distance=mc), repeats)
    ms_eval, ev = _ms(lambda: U.evaluate_registration(da, db, mc, r["transformation"]), repeats)
    ms_total, res = _ms(lambda: U.registration_fgr_based_on_correspondence(da, db, corres, U.FastGlobalRegistrationOption(
        maximum_correspondence_distance=mc)), repeats)
    return {"splats": n_splats, "voxel": voxel, "points": [len(da), len(db)], "reciprocal_pairs": m, "tuple_trials": n_trials,
            "tuples": int(tuples.shape[0]) // 3, "trials_when_none_pass": n_all, "ms_match": ms_match, "ms_tuple_test": ms_tuple,
            "ms_tuple_test_all_trials": ms_tuple_all, "trials_per_s_all_trials": n_all / (ms_tuple_all["device"] * 1e-3),
            "ms_optimize_tuple_list": ms_opt, "ms_optimize_reciprocal_set": ms_opt_full, "iterations": [r["iterations"], rf["iterations"]],
            "ms_evaluate": ms_eval, "ms_fgr_after_matching": ms_total, "fitness": res.fitness,
            "rot_err_deg": G.rotation_error_deg(res.transformation, T), "t_err": float(np.linalg.norm(res.transformation[:3, 3] - T[:3, 3])),
            "rot_err_deg_reciprocal_set": G.rotation_error_deg(rf["transformation"], T)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ransac-iters", type=int, default=100000)
    ap.add_argument("--no-ransac", action="store_true", help="skip the RANSAC stage of scripts/bench_global.py")
    ap.add_argument("--only-large", action="store_true", help="the 100 k case alone (for a profiler run)")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    sizes = [(60000, 0.05), (600000, 0.009)]          # the test scene; about 100 k points per cloud
    if a.only_large:
        sizes = sizes[1:]
    line = {"metric": "Fast Global Registration stages after FPFH, ms (median of %d)" % a.repeats, "fgr": [run(n, v, a.repeats) for n, v in sizes]}
    if not a.no_ransac:
        import bench_global
        rs = [bench_global.run_gpu(n, v, a.ransac_iters, 3) for n, v in sizes]
        line["ransac"] = [{"splats": r["splats"], "points": r["points"], "corres": r["corres"], "hypotheses": r["hypotheses"],
                           "ms_ransac": r["ms_ransac"], "rot_err_deg": r["rot_err_deg"]} for r in rs]
        line["fgr_after_matching_over_ransac"] = [f["ms_fgr_after_matching"]["wall"] / r["ms_ransac"] for f, r in zip(line["fgr"], rs)]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
