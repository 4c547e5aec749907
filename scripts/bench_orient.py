"""Consistent normal orientation on the MI355X: one JSON line with (1) the device time of gsr_orient_normals on the two cloud
sizes of scripts/bench_global.py (about 20 k and 100 k points after the voxel grid; radius = 2 * voxel, max_nn = 30), split by the
call's own events into lists / CSR and weights / Boruvka rounds / vote and flip, next to the same run's gsr_hybrid_search and
gsr_fpfh at the FPFH parameters (5 * voxel, 100), and (2) the share of right mutual feature matches with orient="centroid" and
orient="consistent" on the test scene of DESIGN.md section 12 and on a scene that is not star-shaped (a torus beside a sphere).

    python scripts/bench_orient.py [--repeats 7] [--out profiles/orient_bench.json]

Times: two warm-up calls, then `repeats` calls; median, min and max.  "wall" is the host clock around the synchronised call, the
phases are hipEvents on the call's stream.  A mutual match (i, j) is right when |T p_i - q_j| <= 1.5 * voxel for the known motion T.
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


def _stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def _timed(fn, repeats, warmup=2):
    import torch
    out, wall = None, []
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            wall.append(((time.perf_counter() - t0) * 1e3, out))
    return wall


def timing(n_splats, voxel, repeats):
    import torch
    import global_model as G
    from gaussiansplattingregistration_amd import features as F, orient
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    sc = G.make_scene(n_splats, 1)
    d = PointCloud(xyz32=torch.from_numpy(sc["xyz"]).cuda(), cov6=torch.from_numpy(sc["cov6"]).cuda()).voxel_down_sample(voxel)
    d.estimate_normals()
    xyz, nrm = d.xyz32, d.normals
    if not torch.is_tensor(nrm):
        nrm = torch.as_tensor(np.asarray(nrm, np.float64), device=xyz.device)
    c = xyz.double().mean(0).cpu().numpy()
    runs = _timed(lambda: orient.orient_normals(xyz, nrm, 2 * voxel, 30, reference=c, with_component=False)[1], repeats)
    info = runs[-1][1]
    out = {"splats": n_splats, "voxel": voxel, "points": len(d), "radius": 2 * voxel, "max_nn": 30, "rounds": info["rounds"],
           "n_components": info["n_components"], "n_flipped": info["n_flipped"], "workspace_bytes": info["workspace_bytes"],
           "orient_wall_ms": _stats(w for w, _ in runs),
           "orient_device_ms": _stats(sum(i["phase_ms"].values()) for _, i in runs),
           "phase_ms": {k: _stats(i["phase_ms"][k] for _, i in runs) for k in info["phase_ms"]}}
    out["hybrid_search_fpfh_params_wall_ms"] = _stats(w for w, _ in _timed(lambda: F.hybrid_search(xyz, 5 * voxel, 100), repeats))
    out["hybrid_search_orient_params_wall_ms"] = _stats(w for w, _ in _timed(lambda: F.hybrid_search(xyz, 2 * voxel, 30), repeats))
    oriented = orient.orient_normals(xyz, nrm, 2 * voxel, 30, reference=c, with_component=False)[0]
    out["fpfh_wall_ms"] = _stats(w for w, _ in _timed(lambda: F.fpfh(xyz, oriented, 5 * voxel, 100), repeats))
    return out


def torus_and_sphere(n, seed):
    """a scene the centroid rule splits: a torus (R 1) whose tube radius (0.35) swells and shrinks along it, so that its points do
    not all look alike to FPFH, with a sphere (radius 0.4) beside it; points only -> (points, outward normals)"""
    rng = np.random.default_rng(seed)
    m = int(n * 0.8)
    u, v = rng.uniform(0, 2 * np.pi, m), rng.uniform(0, 2 * np.pi, m)
    r = 0.35 * (1.0 + 0.25 * np.sin(3 * u + 0.5) * np.cos(2 * v) + 0.15 * np.cos(5 * u - v))
    ring = np.stack([np.cos(u), np.sin(u), np.zeros(m)], 1)
    out = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)      # (of the round tube: the sign is what matters)
    t = ring + r[:, None] * out
    so = rng.normal(size=(n - m, 3))
    so /= np.linalg.norm(so, axis=1, keepdims=True)
    s = 0.4 * so + np.array([1.9, 0.3, 0.5])
    return np.concatenate([t, s]) + 0.002 * rng.normal(size=(n, 3)), np.concatenate([out, so])


def _share(make_cloud, T, voxel, orient_mode):
    from gaussiansplattingregistration_amd import features as F
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    downs, feats = [], []
    truth_share = []
    for k in (0, 1):
        pcd, truth_xyz, truth_nrm = make_cloud(k)
        if orient_mode == "none":                                     # the eigen-solver's signs: the reference's behaviour
            d = pcd.voxel_down_sample(voxel)
            d.estimate_normals()
            f = U.compute_fpfh_feature(d, U.KDTreeSearchParamHybrid(5 * voxel, 100))
        else:
            d, f = U.preprocess_point_cloud(pcd, voxel, orient=orient_mode)
        downs.append(d)
        feats.append(f)
        # how many normals look the way the generator's surface normal of the nearest input point looks
        from scipy.spatial import cKDTree
        near = cKDTree(truth_xyz).query(d.points)[1]
        nrm = d.normals.cpu().numpy() if hasattr(d.normals, "cpu") else np.asarray(d.normals)
        truth_share.append(float(((nrm * truth_nrm[near]).sum(1) > 0).mean()))
    corres, used = F.feature_match(feats[0].rows, feats[1].rows, mutual=True)
    corres = corres.cpu().numpy() if hasattr(corres, "cpu") else np.asarray(corres)
    p, q = downs[0].points[corres[:, 0]], downs[1].points[corres[:, 1]]
    err = np.linalg.norm(p @ T[:3, :3].T + T[:3, 3] - q, axis=1)
    out = {"points": [len(downs[0]), len(downs[1])], "mutual_matches": int(corres.shape[0]), "used_mutual": bool(used),
           "right": int((err <= 1.5 * voxel).sum()), "share_right": float((err <= 1.5 * voxel).mean()) if corres.shape[0] else 0.0,
           "share_along_generator_normal": truth_share}
    if orient_mode == "consistent":
        out["components"] = [int(d.orient_info["n_components"]) for d in downs]
        out["rounds"] = [int(d.orient_info["rounds"]) for d in downs]
    return out


def matching():
    import global_model as G
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    T = G.make_T()
    voxel = 0.05
    a, b = G.make_scene(60000, 1), G.transform_scene(G.make_scene(60000, 2), T)
    scene = lambda k: (PointCloud(xyz32=(a, b)[k]["xyz"].astype(np.float32), cov6=(a, b)[k]["cov6"].astype(np.float32)),
                       (a, b)[k]["xyz"].astype(np.float64), (a, b)[k]["normals"])
    ta, na = torus_and_sphere(50000, 1)
    tb, nb = torus_and_sphere(50000, 2)
    tb, nb = tb @ T[:3, :3].T + T[:3, 3], nb @ T[:3, :3].T
    torus = lambda k: (PointCloud(xyz32=(ta, tb)[k].astype(np.float32)), (ta, tb)[k], (na, nb)[k])      # no covariances: KNN-30 normals
    out = {"voxel": voxel, "right_if_within": 1.5 * voxel}
    for name, make in (("section12_scene", scene), ("torus_and_sphere", torus)):
        out[name] = {mode: _share(make, T, voxel, mode) for mode in ("none", "centroid", "consistent")}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("--repeats must be at least 5")
    import __graft_entry__ as g
    g.build_hip()
    line = {"metric": "consistent normal orientation: device ms per cloud and share of right mutual FPFH matches",
            "timing": [timing(n, v, a.repeats) for n, v in ((200000, 0.02), (600000, 0.009))], "matching": matching()}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
