"""Global registration on the MI355X: one JSON line with the time of each stage of do_ransac_registration on two scene sizes
(about 20 k and 100 k points after down-sampling), and the NumPy restatement's time for the same stages at a size it finishes.

    python scripts/bench_global.py [--repeats 3] [--ransac-iters 100000]

Stages (device milliseconds, wall clock around each library call after a warm-up run): preprocessing (voxel down-sampling +
normals + orientation, both clouds), FPFH (both clouds), matching (mutual), RANSAC (edge-length 0.9 + distance 1.5 voxel checkers,
confidence 1.0 so that every hypothesis is evaluated: max_iteration hypotheses).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _ms(fn, repeats):
    import torch
    best = None
    out = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def run_gpu(n_splats, voxel, iters, repeats):
    import torch
    import global_model as G
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    T = G.make_T()
    a, b = G.make_scene(n_splats, 1), G.transform_scene(G.make_scene(n_splats, 2), T)
    ca = PointCloud(xyz32=torch.from_numpy(a["xyz"]).cuda(), cov6=torch.from_numpy(a["cov6"]).cuda())
    cb = PointCloud(xyz32=torch.from_numpy(b["xyz"]).cuda(), cov6=torch.from_numpy(b["cov6"]).cuda())

    def pre():
        out = []
        for c in (ca, cb):
            d = c.voxel_down_sample(voxel)
            d.estimate_normals()
            out.append(U.orient_normals_towards_centroid(d))
        return out
    ms_pre, (da, db) = _ms(pre, repeats)
    prm = U.KDTreeSearchParamHybrid(5 * voxel, 100)
    ms_fpfh, (fa, fb) = _ms(lambda: (U.compute_fpfh_feature(da, prm), U.compute_fpfh_feature(db, prm)), repeats)
    from gaussiansplattingregistration_amd import features as F
    ms_match, (corres, used) = _ms(lambda: F.feature_match(fa.rows, fb.rows, mutual=True), repeats)
    chk = [U.CorrespondenceCheckerBasedOnEdgeLength(0.9), U.CorrespondenceCheckerBasedOnDistance(1.5 * voxel)]
    ms_ransac, r = _ms(lambda: U.registration_ransac_based_on_correspondence(da, db, corres, 1.5 * voxel, None, 3, chk,
                                                                            U.RANSACConvergenceCriteria(iters, 1.0)), repeats)
    n_h = r.info["n_evaluated"]
    return {"splats": n_splats, "voxel": voxel, "points": [len(da), len(db)], "corres": int(corres.shape[0]), "used_mutual": bool(used),
            "ms_preprocess": ms_pre, "ms_fpfh": ms_fpfh, "ms_match": ms_match, "ms_ransac": ms_ransac, "hypotheses": n_h,
            "hypotheses_per_s": n_h / (ms_ransac * 1e-3), "valid_hypotheses": r.info["n_valid"], "fitness": r.fitness,
            "rot_err_deg": G.rotation_error_deg(r.transformation, T),
            "t_err": float(np.linalg.norm(r.transformation[:3, 3] - T[:3, 3]))}


def run_numpy(n_splats, voxel, iters):
    import global_model as G
    T = G.make_T()
    a, b = G.make_scene(n_splats, 1), G.transform_scene(G.make_scene(n_splats, 2), T)
    t0 = time.perf_counter()
    clouds = []
    for sc in (a, b):
        P, C = G.voxel_down(sc["xyz"], sc["cov6"], voxel)
        N = G.normals_from_cov(C)
        N = np.where(((P.mean(0) - P) * N).sum(1, keepdims=True) < 0, -N, N)
        clouds.append((P.astype(np.float32), N))
    t1 = time.perf_counter()
    feats = [G.spfh_fpfh(x, n, 5 * voxel, 100)[1] for x, n in clouds]
    t2 = time.perf_counter()
    corres, _, _, _ = G.feature_match(feats[0], feats[1], True)
    t3 = time.perf_counter()
    r = G.ransac(clouds[0][0], clouds[1][0], corres, 1.5 * voxel, checkers=[(G.EDGE, 0.9), (G.DIST, 1.5 * voxel)], max_iteration=iters,
                 confidence=1.0, batch=1024)
    t4 = time.perf_counter()
    return {"splats": n_splats, "voxel": voxel, "points": [len(c[0]) for c in clouds], "ms_preprocess": (t1 - t0) * 1e3,
            "ms_fpfh": (t2 - t1) * 1e3, "ms_match": (t3 - t2) * 1e3, "ms_ransac": (t4 - t3) * 1e3, "hypotheses": r["n_evaluated"],
            "hypotheses_per_s": r["n_evaluated"] / (t4 - t3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ransac-iters", type=int, default=100000)
    ap.add_argument("--numpy-iters", type=int, default=2000)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    # two scene sizes: ~20 k and ~100 k points per cloud after down-sampling
    sizes = [(200000, 0.02), (600000, 0.009)]
    gpu = [run_gpu(n, v, a.ransac_iters, a.repeats) for n, v in sizes]
    line = {"metric": "global registration stages (FPFH + mutual matching + RANSAC), ms", "gpu": gpu}
    if not a.no_numpy:
        line["numpy_restatement"] = run_numpy(60000, 0.05, a.numpy_iters)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
