"""Photometric refinement on the MI355X: writes ``profiles/photo_bench.json`` and prints it as one JSON line.

    python scripts/bench_photo.py [--repeats 5] [--splats 1000000] [--cameras 8] [--out profiles/photo_bench.json]

``accumulate``: ``gsr_photo_accumulate`` on device maps at 1280 x 720 and 1920 x 1080 beside ``gsr_image_metrics`` on images of the same
size in the same session -- the yardstick: both are one streaming pass over image maps with a float64 fold.  Milliseconds between two
events on the stream around the call (the kernels and the read-back of the sums), median of ``--repeats`` after a warm-up call; the
bytes are what the kernel must read (40 per pixel: two colour, two depth and two coverage maps; 24 per pixel for the metrics).

``refine``: one whole ``PhotometricRefiner.run()`` of the 2 x ``--splats`` pair (the bench cloud and the same cloud moved) over
``--cameras`` 1280 x 720 views on a circle around the box, started a small rigid motion off the truth: wall clock, the renders included.
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


def _event_ms(call, repeats):
    import torch
    call()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), out


def accumulate_case(width, height, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import photo, raster
    from gaussiansplattingregistration_amd.params import PhotometricParams
    g = torch.Generator(device="cuda:0").manual_seed(width)
    y, x = torch.meshgrid(torch.arange(height, device="cuda:0", dtype=torch.float32), torch.arange(width, device="cuda:0", dtype=torch.float32), indexing="ij")

    def maps(k):
        img = torch.stack([0.5 + 0.3 * torch.sin(0.03 * x + 0.02 * y + c + 0.05 * k) for c in range(3)], -1) + 0.02 * torch.randn((height, width, 3), generator=g, device="cuda:0")
        depth = 2.0 + 0.3 * torch.sin(0.021 * x + 0.4) * torch.cos(0.017 * y) + 0.05 * k * torch.rand((height, width), generator=g, device="cuda:0")
        alpha = torch.where(torch.rand((height, width), generator=g, device="cuda:0") < 0.02, 0.1, 0.9) * torch.ones_like(depth)
        return dict(image=img.contiguous(), depth=depth.contiguous(), alpha=alpha.contiguous())
    src, tgt = maps(0), maps(1)
    V = np.eye(4)
    V[2, 3] = 2.5
    cam = photo.PhotoCamera(V, 1.1 * width, 1.1 * width, width / 2, height / 2, width, height)
    P = PhotometricParams(max_depth_diff=0.25)
    sums = photo.accumulate_sums(src, tgt, cam, P)
    ms_a, all_a = _event_ms(lambda: photo.accumulate_sums(src, tgt, cam, P), repeats)
    a, b = src["image"].permute(2, 0, 1).contiguous(), tgt["image"].permute(2, 0, 1).contiguous()
    ms_m, all_m = _event_ms(lambda: raster.image_metrics(a, b), repeats)
    px = width * height
    return {"width": width, "height": height, "counted_pixels": int(sums[29]), "ms_photo_accumulate": ms_a, "ms_photo_accumulate_all": all_a,
            "ms_image_metrics": ms_m, "ms_image_metrics_all": all_m, "photo_bytes_read": 40 * px, "metrics_bytes_read": 24 * px,
            "photo_GBps": 40 * px / (ms_a * 1e-3) / 1e9, "metrics_GBps": 24 * px / (ms_m * 1e-3) / 1e9, "ratio_photo_over_metrics": ms_a / ms_m}


def refine_case(n, cameras, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import photo, synth
    from gaussiansplattingregistration_amd.models.camera import Camera
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import PhotometricParams
    a = synth.make_cloud_torch(n, seed=1, device="cuda:0", sh_degree=3)
    T_gt = synth.rigid_transform(5.0, (1, 1, 1), (0.1, -0.1, 0.05))
    b = synth.apply_rigid_torch(a, T_gt)
    h = float(a["h"])
    model = lambda m: GaussianModel("cuda:0").from_arrays(m["xyz"], m["color"], m["opacity"], m["cov6"], m["sh"], 3)
    source, target = model(a), model(b)
    cams = []
    for k in range(cameras):
        ang = 2.0 * np.pi * k / cameras
        eye = 4.0 * h * np.array([np.sin(ang), 0.0, -np.cos(ang)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])               # world -> camera
        cams.append(Camera(R.T, -R @ eye, 1100.0, 1155.0, f"ring_{k}", 1280, 720))
    init = photo.se3_exp(np.array([0.004, -0.003, 0.005, 0.01 * h, -0.008 * h, 0.006 * h])) @ T_gt
    P = PhotometricParams(max_depth_diff=0.5 * h)
    run = lambda: photo.PhotometricRefiner(source, target, cams, P, init=init).run()
    r = run()
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    err = lambda T: (float(np.linalg.norm((T @ np.linalg.inv(T_gt))[:3, 3])), float(np.linalg.norm((T @ np.linalg.inv(T_gt))[:3, :3] - np.eye(3))))
    return {"splats": 2 * n, "cameras": cameras, "width": 1280, "height": 720, "h": h, "ms_wall": statistics.median(wall), "ms_wall_all": wall,
            "iterations": r.iterations, "source_renders": (r.iterations + len(r.trace) + 2) * cameras, "energy_initial": r.energy_initial,
            "energy_final": r.energy_final, "n_pixels": r.n_pixels, "error_initial": err(init), "error_final": err(np.asarray(r.transformation)),
            "levels": [{k: row[k] for k in ("scale", "width", "height", "iterations", "accepted", "n_pixels")} for row in r.trace], "error_list": r.error_list}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--splats", type=int, default=1_000_000, help="per cloud of the refined pair")
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--skip-refine", action="store_true", help="the accumulate cases alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    result = {"metric": "photometric refinement, ms (median of %d after a warm-up)" % a.repeats,
              "accumulate": [accumulate_case(1280, 720, a.repeats), accumulate_case(1920, 1080, a.repeats)]}
    if not a.skip_refine:
        result["refine"] = refine_case(a.splats, a.cameras, a.repeats)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
