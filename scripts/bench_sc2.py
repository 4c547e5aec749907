"""Compatibility-graph global registration (csrc/sc2.hip) on the MI355X: the time of each stage of gsr_sc2_correspondence at the two
scene sizes of scripts/bench_global.py, and gsr_ransac_correspondence at 100 000 hypotheses with confidence 1 on the same
correspondences in the same run as the yardstick.  Writes profiles/sc2_bench.json and prints it as one JSON line.

    python scripts/bench_sc2.py [--repeats 7] [--warmup 2] [--ransac-iters 100000] [--out profiles/sc2_bench.json]

Whole calls are timed with stream events around the call (device arrays, the call's own waits included); the stages with the
stream events gsr_test_sc2_timed records between them in those same calls.  The two methods alternate, SC2 then RANSAC, `repeats`
times after `warmup` untimed rounds; every figure is the median with the smallest and largest value beside it.  A guard: should a
scene's mutual matches exceed GSR_SC2_MAX_CORRES, an evenly strided subset of that size is used for both methods and both counts
are reported (`mutual_matches`, `corres`); at the two sizes here it is not triggered (3 944 and 11 933 matches).
MAC/s of k_sc2_rows = n_seeds * m * m (the products the definition needs, not the padded tile's) over the stage's time.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("compat", "seed_sort", "rows", "sets", "score", "refine")


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(n_splats, voxel, iters, repeats, warmup):
    import torch
    import global_model as G
    from gaussiansplattingregistration_amd import _lib, _marshal as _m, features as F
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    L = _lib.load(require_device=True)
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
    corres, used = F.feature_match(fa.rows, fb.rows, mutual=True)
    m_all = int(corres.shape[0])
    if m_all > _lib.GSR_SC2_MAX_CORRES:
        keep = torch.linspace(0, m_all - 1, _lib.GSR_SC2_MAX_CORRES, device=corres.device).round().long()
        corres = corres[keep].contiguous()
    m = int(corres.shape[0])
    d_thr = 1.5 * voxel
    xs, xt = da.xyz32.contiguous(), db.xyz32.contiguous()
    P = F._sc2_params(d_thr, 0.2, 4096, 30, 20, 20)
    chk = [(F.CHECK_EDGE_LENGTH, 0.9), (F.CHECK_DISTANCE, d_thr)]
    stream = C.c_void_p(_m.stream_ptr(0, True))
    ms_sc2, ms_ransac, ms_stage = [], [], {k: [] for k in STAGES}
    R, r = _lib.Sc2Result(), None
    for it in range(warmup + repeats):
        st = np.zeros(len(STAGES), np.float32)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        _lib.check(L.gsr_test_sc2_timed(xs.data_ptr(), xs.shape[0], xt.data_ptr(), xt.shape[0], corres.data_ptr(), m, C.byref(P), C.byref(R),
                                        st.ctypes.data, 1, 0, stream), "gsr_test_sc2_timed")
        e1.record()
        r = F.ransac_correspondence(xs, xt, corres, d_thr, checkers=chk, max_iteration=iters, confidence=1.0)
        e2.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms_sc2.append(e0.elapsed_time(e1))
            ms_ransac.append(e1.elapsed_time(e2))
            for k, v in zip(STAGES, st):
                ms_stage[k].append(float(v))
    s = F._sc2_dict(R)
    stages = {k: _stat(v) for k, v in ms_stage.items()}
    largest = max(STAGES, key=lambda k: stages[k]["median"])
    macs = float(s["n_seeds"]) * m * m
    return {"splats": n_splats, "voxel": voxel, "points": [int(xs.shape[0]), int(xt.shape[0])], "mutual_matches": m_all, "corres": m,
            "used_mutual": bool(used), "d_thr": d_thr, "repeats": repeats, "warmup": warmup,
            "sc2": {"ms_call": _stat(ms_sc2), "ms_stage": stages, "largest_stage": largest, "rows_is_largest_stage": largest == "rows",
                    "rows_macs": macs, "rows_mac_per_s": macs / (stages["rows"]["median"] * 1e-3),
                    "C_bytes": int(-(-m // 128) * 128) * int(-(-m // 64) * 64), "n_seeds": s["n_seeds"], "n_valid": s["n_valid"],
                    "n_edges": s["n_edges"], "refine_steps": s["refine_steps"], "host_waits": s["host_waits"], "fitness": s["fitness"],
                    "rot_err_deg": G.rotation_error_deg(s["transformation"], T),
                    "t_err": float(np.linalg.norm(s["transformation"][:3, 3] - T[:3, 3]))},
            "ransac": {"ms_call": _stat(ms_ransac), "hypotheses": r["n_evaluated"], "valid_hypotheses": r["n_valid"], "fitness": r["fitness"],
                       "checkers": "edge length 0.9, distance d_thr", "rot_err_deg": G.rotation_error_deg(r["transformation"], T),
                       "t_err": float(np.linalg.norm(r["transformation"][:3, 3] - T[:3, 3]))}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ransac-iters", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sc2_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    sizes = [(200000, 0.02), (600000, 0.009)]                  # the two of scripts/bench_global.py
    line = {"metric": "compatibility-graph global registration: stages of gsr_sc2_correspondence and the RANSAC yardstick, ms (stream events)",
            "sizes": [run(n, v, a.ransac_iters, a.repeats, a.warmup) for n, v in sizes]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
