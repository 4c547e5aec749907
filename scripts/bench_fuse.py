"""The overlap-aware merge (GaussianModel.fuse_overlap, gsr_model_fuse) on the MI355X, measured: writes profiles/fuse_bench.json.

    python scripts/bench_fuse.py [--sizes 1000000 5000000] [--repeats 5] [--out profiles/fuse_bench.json]

Per size n: the pair of synth.make_pair(n) (SH degree 3), the source moved into the target's frame by the known transform
(transform_gaussian_model, rotate_sh=True), then fused with the target under max_distance = 2 x the median nearest-neighbour spacing
of the target and the default kld_max (no colour gate).  Recorded: the milliseconds per phase by the library's device events (pre-pass
and grid, search, pairs and scans, writer; medians over the repeats after one warm-up call), the wall clock of the call (the output
allocation, both host waits), n_pairs, the gated pairs, and the plain merge (torch.cat of the same two models) beside it.
`algorithmic_bytes` = every input row read once and every output row written once (232 bytes per row at degree 3);
`fraction_of_hbm_peak` = those bytes over the sum of the four phases over 8.0 TB/s.  No threshold: this records what is seen.
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
HBM_PEAK = 8.0e12          # bytes per second, the MI355X's specification


def median_nn_spacing(xyz, h):
    """median nearest-neighbour distance of the cloud, from the points of its central part (the density is uniform)"""
    import numpy as np
    from scipy.spatial import cKDTree
    sub = xyz[(np.abs(xyz) < 0.4 * h).all(1)].astype(np.float64)
    inner = sub[(np.abs(sub) < 0.35 * h).all(1)]
    d, _ = cKDTree(sub).query(inner, k=2, workers=8)
    return float(np.median(d[:, 1]))


def run(n, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import FuseOverlapParams
    src, tgt, T_gt = synth.make_pair(n, seed=5)
    spacing = median_nn_spacing(tgt["xyz"], tgt["h"])
    params = FuseOverlapParams(max_distance=2.0 * spacing)
    model = lambda c: GaussianModel("cuda:0").from_arrays(c["xyz"], c["color"], c["opacity"].reshape(-1, 1), c["cov6"], c["sh"].reshape(n, 15, 3), 3)
    g1 = model(src).transform_gaussian_model(T_gt, rotate_sh=True)
    g2 = model(tgt)
    for g in (g1, g2):                      # no scaling / rotation: empty tensors on the models' device, which the plain merge concatenates
        g._scaling = g._rotation = torch.empty(0, device="cuda:0")
    del src, tgt
    torch.cuda.synchronize()
    merged, info = GaussianModel.fuse_overlap(g1, g2, params)          # warm-up: code objects, rocPRIM's choices
    phases, wall, plain = [], [], []
    for _ in range(repeats):
        del merged
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        merged, info = GaussianModel.fuse_overlap(g1, g2, params)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        phases.append(info["phase_ms"])
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cat = GaussianModel.get_merged_gaussian_point_clouds(g1, g2, np.eye(4))
        torch.cuda.synchronize()
        plain.append((time.perf_counter() - t0) * 1e3)
        del cat
    med = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
    row_bytes = 4 * (3 + 6 + 3 + 45 + 1)
    algo = (2 * n + info["n_out"]) * row_bytes
    total = sum(med.values())
    return {"n_a": n, "n_b": n, "sh_degree": 3, "median_nn_spacing": spacing, "max_distance": params.max_distance, "kld_max": params.kld_max,
            "color_delta": "inf", "n_pairs": info["n_pairs"], "n_out": info["n_out"], "gated_pairs": info["gated_pairs"],
            "n_invalid_a": info["n_invalid_a"], "n_invalid_b": info["n_invalid_b"], "phase_ms": med, "phase_ms_sum": total,
            "wall_ms": statistics.median(wall), "wall_ms_all": wall, "plain_merge_wall_ms": statistics.median(plain[1:]), "repeats": repeats,
            "algorithmic_bytes": algo, "fraction_of_hbm_peak": algo / (total * 1e-3) / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 5000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse.py measures on the GPU: no device is visible")
    import __graft_entry__ as g
    g.build_hip()
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "timing": "hipEvents of gsr_model_fuse, medians",
           "cases": [run(n, a.repeats) for n in a.sizes]}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
