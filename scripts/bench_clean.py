"""Floater removal (GaussianModel.remove_floaters: gsr_outlier_mask + gsr_model_select) on the MI355X, measured: writes
profiles/clean_bench.json.

    python scripts/bench_clean.py [--sizes 1000000 5000000] [--floaters 0 0.001 0.01] [--repeats 5] [--out profiles/clean_bench.json]
                                  [--row-limit-s 20]

Per size n and floater fraction f: synth.make_cloud_torch(n) (SH degree 3, drawn on the device) with f n rows moved to 5 - 50 box radii
along random directions, all on the device.  Two parameter sets: the statistical filter alone (k = 20, ratio 2.0), then with the
radius filter (radius = 2 x the median nearest-neighbour spacing of the clean cloud, nb_points 16).  Recorded per row: the milliseconds
per phase by the library's device events (pre-pass + grid, k-NN + moments, radius count, mask; medians over the repeats after one
warm-up call), the wall clock of the mask call and of the selection, deferred_queries, n_kept, and the algorithmic bytes -- 16 B read
and 1 B written per row for the mask, every kept row read once and written once for the selection (232 B per row at degree 3 with
scaling / rotation) -- as a fraction of 8.0 TB/s over the time they took.  Yardstick of the k-NN kernel: gsr_normals_knn(knn = 20), the
library's other k-NN over a whole cloud (the same grid_ring_walk over a GridIndex of its own), on the same 1 M clean cloud in the same
run (wall clock of the call on device tensors, which like the mask call includes the grid build); the ratio is knn_phase_and_grid_ms / normals_knn_ms.  Yardstick of the floater rows: the 0 %
row of the same table.  A row whose warm-up call takes longer than --row-limit-s is recorded with that one time and not repeated, and
larger sizes of the same fraction are skipped (recorded as skipped).  No threshold: this records what is seen.
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


def make_model(n, fraction, seed=1):
    import math
    import torch
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    c = synth.make_cloud_torch(n, seed=seed, device="cuda:0", sh_degree=3)
    g = torch.Generator(device="cuda:0").manual_seed(seed + 77)
    xyz = c["xyz"].clone()
    nf = int(round(fraction * n))
    if nf:
        lo, hi = xyz.min(0).values, xyz.max(0).values
        ctr, rad = 0.5 * (lo + hi), 0.5 * float(torch.linalg.vector_norm(hi - lo))
        d = torch.randn((nf, 3), generator=g, device="cuda:0")
        d = d / torch.linalg.vector_norm(d, dim=1, keepdim=True)
        r = (5.0 + 45.0 * torch.rand((nf, 1), generator=g, device="cuda:0")) * rad
        rows = torch.randperm(n, generator=g, device="cuda:0")[:nf]
        xyz[rows] = (ctr + d * r).float()
    m = GaussianModel("cuda:0").from_arrays(xyz, c["color"], c["opacity"], c["cov6"], c["sh"], 3)
    m._scaling = torch.full((n, 3), math.log(0.01), device="cuda:0")
    m._rotation = torch.zeros((n, 4), device="cuda:0")
    m._rotation[:, 0] = 1.0
    return m, nf


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def measure(model, params, repeats, row_limit_s):
    from gaussiansplattingregistration_amd import clean
    n = len(model)
    call = lambda: clean.outlier_mask(model._xyz, params, raw_opacity=model._opacity.reshape(n), scaling=model._scaling)
    (mask, info), warm_ms = timed(call)
    row = {"n": n, "n_kept": info["n_kept"], "deferred_queries": info["deferred_queries"], "threshold": info["threshold"],
           "dropped": {k: info[k] for k in ("n_nonfinite", "n_gate_opacity", "n_gate_scale", "n_statistical", "n_radius")},
           "workspace_bytes": info["workspace_bytes"], "warmup_wall_ms": warm_ms}
    phases, walls, sel_walls = [info["phase_ms"]], [warm_ms], []
    row["repeated"] = warm_ms <= row_limit_s * 1e3
    if row["repeated"]:
        phases, walls = [], []
        for _ in range(repeats):
            (mask, info), ms = timed(call)
            phases.append(info["phase_ms"])
            walls.append(ms)
    for _ in range(repeats if row["repeated"] else 1):
        cleaned, ms = timed(lambda: model.select_by_mask(mask))
        sel_walls.append(ms)
    med = lambda xs: float(statistics.median(xs))
    row["phase_ms"] = {k: med([p[k] for p in phases]) for k in phases[0]}
    row["mask_wall_ms"], row["select_wall_ms"] = med(walls), med(sel_walls)
    mask_bytes, sel_bytes = 17 * n, 2 * 232 * info["n_kept"]
    mask_ms = sum(row["phase_ms"].values())
    row["algorithmic_bytes"] = {"mask": mask_bytes, "select": sel_bytes}
    row["fraction_of_hbm_peak"] = {"mask": mask_bytes / (mask_ms * 1e-3) / HBM_PEAK if mask_ms > 0 else None,
                                   "select": sel_bytes / (row["select_wall_ms"] * 1e-3) / HBM_PEAK}
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 5000000])
    ap.add_argument("--floaters", type=float, nargs="+", default=[0.0, 0.001, 0.01])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--row-limit-s", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_bench.json"))
    a = ap.parse_args()

    import __graft_entry__ as g
    g.build_hip()
    import torch
    from gaussiansplattingregistration_amd import clean, icp
    from gaussiansplattingregistration_amd.params.clean_parameters import CleanParams

    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": [], "yardstick_knn": None}

    def save():
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    too_slow = set()                      # floater fractions whose last row ran past the limit: larger sizes are skipped
    for n in sorted(a.sizes):
        spacing = None
        for frac in a.floaters:
            if frac in too_slow:
                result["rows"].append({"n": n, "floater_fraction": frac, "skipped": "the smaller size of this fraction ran past --row-limit-s"})
                save()
                continue
            model, nf = make_model(n, frac)
            if spacing is None:           # of the clean cloud (the first fraction is 0): twice the mean over {self, nearest}
                clean_model, _ = (model, nf) if nf == 0 else make_model(n, 0.0)
                _, inf2 = clean.outlier_mask(clean_model._xyz, CleanParams(nb_neighbors=2, std_ratio=2.0), with_mean_dist=True)
                spacing = float(2.0 * torch.median(inf2["mean_dist"]))
                if n == 1000000 and result["yardstick_knn"] is None:
                    times = [timed(lambda: icp.normals_knn(clean_model._xyz, knn=20))[1] for _ in range(a.repeats + 1)][1:]
                    result["yardstick_knn"] = {"n": n, "normals_knn_ms": float(statistics.median(times))}
                del clean_model
            for label, P in (("statistical", CleanParams(nb_neighbors=20, std_ratio=2.0)),
                             ("statistical+radius", CleanParams(nb_neighbors=20, std_ratio=2.0, radius=2.0 * spacing, nb_points=16))):
                row = measure(model, P, a.repeats, a.row_limit_s)
                row.update(floater_fraction=frac, n_floaters=nf, params=label, radius=P.radius, median_nn_spacing=spacing)
                if not row["repeated"]:
                    too_slow.add(frac)
                if result["yardstick_knn"] and n == result["yardstick_knn"]["n"] and frac == 0.0 and label == "statistical":
                    y = result["yardstick_knn"]
                    y["knn_phase_and_grid_ms"] = row["phase_ms"]["prepass_grid"] + row["phase_ms"]["knn"]
                    y["knn_phase_ms"] = row["phase_ms"]["knn"]
                    y["ratio"] = y["knn_phase_and_grid_ms"] / y["normals_knn_ms"]
                result["rows"].append(row)
                print(json.dumps({k: row[k] for k in ("n", "floater_fraction", "params", "n_kept", "deferred_queries", "phase_ms", "mask_wall_ms",
                                                      "select_wall_ms")}), flush=True)
                save()
            del model
            torch.cuda.empty_cache()
    save()
    print("->", a.out)


if __name__ == "__main__":
    main()
