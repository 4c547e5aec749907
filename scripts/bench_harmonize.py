"""Colour harmonisation (GaussianModel.match_colors; gsr_model_match, gsr_color_sums, gsr_model_color_apply) on the MI355X, measured:
writes profiles/harmonize_bench.json.

    python scripts/bench_harmonize.py [--sizes 1000000 5000000] [--repeats 5] [--out profiles/harmonize_bench.json]

Per size n: the pair of synth.make_pair(n) (SH degree 3), the source moved into the target's frame by the known transform
(transform_gaussian_model, rotate_sh=True) and its colours distorted by a known affine transform.  Recorded, each the median of the
repeats after one warm-up call, with the smallest and the largest:
  match_ms        one gsr_model_match under max_distance = 2 x the expected nearest-neighbour spacing, by device events around the call
  sums_ms         one gsr_color_sums over its pairs (Huber 0.1, identity transforms), likewise
  apply_ms        one gsr_model_color_apply of the source (out of place), likewise
  copy_ms         a device-to-device copy of the bytes the apply kernel moves (n (3 + 3 K) 4 in, the same out): its yardstick
  match_colors_s  the wall clock of the whole GaussianModel.match_colors (pair list, 5 + 1 rounds of sums, 5 solves)
and the coefficient error of the fitted transform against the known one.  No target: no earlier figure exists.
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


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(n, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import harmonize, synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import ColorMatchParams, FuseOverlapParams
    src, tgt, T_gt = synth.make_pair(n, seed=5)
    spacing = 0.554 * (2.0 * tgt["h"]) / n ** (1.0 / 3.0)          # mean nearest-neighbour distance of a uniform cloud
    gate = FuseOverlapParams(max_distance=2.0 * spacing)
    K = 15
    model = lambda c: GaussianModel("cuda:0").from_arrays(c["xyz"], c["color"], c["opacity"].reshape(-1, 1), c["cov6"], c["sh"].reshape(n, K, 3), 3)
    rng = np.random.default_rng(17)
    D = harmonize.IDENTITY + rng.uniform(-0.15, 0.15, (3, 4))                       # the source's fitted transform
    Dinv = np.linalg.inv(np.vstack([D, [0, 0, 0, 1]]))[:3]
    g1 = model(src).transform_gaussian_model(T_gt, rotate_sh=True).apply_color_transform(Dinv)
    g2 = model(tgt)
    del src, tgt
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()                                                                        # warm-up: code objects, rocPRIM's choices
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            a.record()
            r = fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return stat(out), r

    match_ms, (pairs, rep) = timed(lambda: harmonize.match_pairs(g1, g2, gate))
    dc1, op1 = g1._features_dc.reshape(n, 3), g1._opacity.reshape(n)
    dc2, op2 = g2._features_dc.reshape(n, 3), g2._opacity.reshape(n)
    sums_ms, (S, sinfo) = timed(lambda: harmonize.color_sums(dc1, op1, dc2, op2, pairs, huber=0.1))
    apply_ms, _ = timed(lambda: harmonize.apply_color_arrays(D, g1._features_dc, g1._features_rest))
    moved = n * (3 + 3 * K) * 4
    a = torch.empty(moved // 4, dtype=torch.float32, device="cuda:0").normal_()
    b = torch.empty_like(a)
    copy_ms, _ = timed(lambda: b.copy_(a))
    del a, b
    params = ColorMatchParams()
    walls = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P, info = GaussianModel.match_colors([g1, g2], gate, params, edges=[(0, 1)], reference=1)
        torch.cuda.synchronize()
        if i:
            walls.append(time.perf_counter() - t0)
    e = info["edges"][0]
    return {"n": n, "sh_degree": 3, "max_distance": gate.max_distance, "n_pairs": int(rep["n_pairs"]), "n_skipped": sinfo["n_skipped"],
            "match_ms": match_ms, "match_phase_ms": rep["phase_ms"], "match_workspace_bytes": rep["workspace_bytes"], "sums_ms": sums_ms,
            "apply_ms": apply_ms, "copy_ms": copy_ms, "apply_bytes_in": moved, "apply_bytes_out": moved,
            "apply_over_copy": apply_ms["median"] / copy_ms["median"],
            "apply_GBps": 2 * moved / (apply_ms["median"] * 1e-3) / 1e9, "copy_GBps": 2 * moved / (copy_ms["median"] * 1e-3) / 1e9,
            "match_colors_s": stat(walls), "rms_before": e["rms_before"], "rms_after": e["rms_after"],
            "coefficient_error": float(np.abs(P[0] - D).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 5000000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmonize_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for n in a.sizes:
        rows.append(run(n, a.repeats))
        print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "statistic": "median of the repeats after one warm-up, with min and max",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
