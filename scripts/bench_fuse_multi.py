"""The N-way overlap merge (GaussianModel.fuse_overlap_multi, gsr_fuse_multi) on the MI355X, measured: writes
profiles/fuse_multi_bench.json.

    python scripts/bench_fuse_multi.py [--cases 2x1000000 4x1000000 8x1000000 4x5000000] [--repeats 5] [--out profiles/fuse_multi_bench.json]

Per case NxR: N noisy copies of synth.make_cloud(R) (SH degree 3; copy 0 is the cloud, every other copy has 0.002 of position noise, as
synth.make_pair's jitter), fused under max_distance = 2 x the median nearest-neighbour spacing of the cloud and the default kld_max (no
colour gate).  Recorded, medians over the repeats after one warm-up call: the milliseconds per phase by the library's device events
(pre-pass and grid, search, edge list, rounds, ranks and writer), the wall clock of the call, the number of rounds, and from the same
run (a) the plain merge (get_merged_gaussian_point_clouds_multi with identity poses: allocate once, copy), (b) the fold of N - 1
pairwise GaussianModel.fuse_overlap calls (gsr_model_fuse, whose kernels and results this library shares with its predecessor), which
for N = 2 is (c) gsr_model_fuse itself.  `algorithmic_bytes` = every input row read once and every output row written once (232 bytes
per row at degree 3); `fraction_of_hbm_peak` = those bytes over the sum of the phases over 8.0 TB/s.  A case that does not fit the
device's memory is recorded as skipped.  No threshold: this records what is seen.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12          # bytes per second, the MI355X's specification


def run(N, n, repeats):
    import numpy as np
    import torch
    from bench_fuse import median_nn_spacing
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import FuseOverlapParams
    h = synth.half_extent(n)
    c = synth.make_cloud(n, seed=5, h=h)
    spacing = median_nn_spacing(c["xyz"], h)
    params = FuseOverlapParams(max_distance=2.0 * spacing)
    base = GaussianModel("cuda:0").from_arrays(c["xyz"], c["color"], c["opacity"].reshape(-1, 1), c["cov6"], c["sh"].reshape(n, 15, 3), 3)
    base._scaling = base._rotation = torch.empty(0, device="cuda:0")      # no scaling / rotation, as in bench_fuse.py
    del c
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(11)
    models = [base]
    for _ in range(1, N):
        g = base.clone_gaussian()
        g._xyz = base._xyz + 0.002 * torch.randn(base._xyz.shape, generator=gen, device="cuda:0")
        g._scaling = g._rotation = torch.empty(0, device="cuda:0")
        models.append(g)
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def fold():
        acc, infos = models[0], []
        for g in models[1:]:
            acc, info = GaussianModel.fuse_overlap(acc, g, params)
            infos.append(info)
        return acc, infos
    eye = [np.eye(4)] * N
    timed(lambda: GaussianModel.fuse_overlap_multi(models, params))          # warm-up: code objects, rocPRIM's choices
    timed(fold)
    timed(lambda: GaussianModel.get_merged_gaussian_point_clouds_multi(models, eye))
    wall, phases, fold_wall, fold_phase_sum, cat_wall = [], [], [], [], []
    for _ in range(repeats):
        ms, (merged, info) = timed(lambda: GaussianModel.fuse_overlap_multi(models, params))
        wall.append(ms)
        phases.append(info["phase_ms"])
        del merged
        ms, (acc, infos) = timed(fold)
        fold_wall.append(ms)
        fold_phase_sum.append(sum(sum(i["phase_ms"].values()) for i in infos))
        fold_out = len(acc)
        del acc
        ms, cat = timed(lambda: GaussianModel.get_merged_gaussian_point_clouds_multi(models, eye))
        cat_wall.append(ms)
        del cat
    med = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
    total = sum(med.values())
    row_bytes = 4 * (3 + 6 + 3 + 45 + 1)
    algo = (N * n + info["n_out"]) * row_bytes
    out = {"n_models": N, "rows_per_model": n, "sh_degree": 3, "median_nn_spacing": spacing, "max_distance": params.max_distance, "kld_max": params.kld_max,
           "color_delta": "inf", "repeats": repeats, "phase_ms": med, "phase_ms_sum": total, "wall_ms": statistics.median(wall), "wall_ms_all": wall,
           "algorithmic_bytes": algo, "fraction_of_hbm_peak": algo / (total * 1e-3) / HBM_PEAK,
           "plain_merge_wall_ms": statistics.median(cat_wall), "pairwise_fold_wall_ms": statistics.median(fold_wall),
           "pairwise_fold_phase_ms_sum": statistics.median(fold_phase_sum), "pairwise_fold_n_out": fold_out,
           "wall_over_plain_merge": statistics.median(wall) / statistics.median(cat_wall),
           "wall_over_pairwise_fold": statistics.median(wall) / statistics.median(fold_wall),
           "phases_over_pairwise_fold_phases": total / statistics.median(fold_phase_sum)}
    for k in ("n_out", "n_groups", "n_grouped_rows", "n_invalid", "gated_pairs", "mutual_edges", "rejected_edges", "rounds", "workspace_bytes", "groups_of_size"):
        out[k] = info[k]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["2x1000000", "4x1000000", "8x1000000", "4x5000000"], metavar="NxROWS")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_multi_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse_multi.py measures on the GPU: no device is visible")
    import __graft_entry__ as g
    g.build_hip()
    cases = []
    for spec in a.cases:
        N, n = (int(x) for x in spec.split("x"))
        try:
            cases.append(run(N, n, a.repeats))
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
            if "out of memory" not in str(e).lower():
                raise
            cases.append({"n_models": N, "rows_per_model": n, "skipped": "out of device memory"})
            torch.cuda.empty_cache()
        print(json.dumps(cases[-1]), flush=True)
        out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
               "timing": "hipEvents of gsr_fuse_multi and gsr_model_fuse, wall clocks with a device synchronisation on both sides; medians", "cases": cases}
        with open(a.out, "w") as f:                         # after every case: a long run that is cut short keeps what it measured
            json.dump(out, f, indent=1)
            f.write("\n")

if __name__ == "__main__":
    main()
