"""The splat rasteriser on the MI355X: one JSON line with the milliseconds per image of the merged bench pair (2 x 5 M splats, SH
degree 3) at 1920 x 1080 from a camera outside the box, split into preprocess / sort / blend (device events of the library), the
wall clock per image, intersections and splats per second; and the same for the 2 x 1 M pair at 1280 x 720.

    python scripts/bench_raster.py [--repeats 5] [--splats 5000000] [--small-only] [--aux]

``ms_per_image_wall`` is ``RasterContext.render`` on ready-made tensors; ``ms_per_image_wall_rasterize_image`` is the reference-named
``rasterize_image`` on a ``GaussianModel``, which also expands and re-packs the covariances on every call.  After one warm-up render (the
workspaces grow once).  ``sort`` contains the call's single host wait (the intersection total).

``--aux`` adds, per case, the same event split for ``render_aux`` with depth + alpha, with the contribution alone and
with every output, under ``aux``; and for the 2 x 1 M case ``prune_unseen`` over 8 cameras on a circle around the box (wall clock of
the eight renders into one buffer, the selection included).
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


def camera_on_the_z_axis(distance, width, height, focal):
    """world -> camera matrix and intrinsics of a camera at (0, 0, -distance) looking at the origin (+z forward, +y down)"""
    import numpy as np
    V = np.eye(4, dtype=np.float32)
    V[2, 3] = distance
    return dict(viewmat=V, fx=float(focal), fy=float(focal) * 1.05, cx=width / 2.0, cy=height / 2.0)


def aux_cases(ctx, m, n, cam, width, height, repeats):
    """the event split of render_aux per set of outputs, after one warm-up each: name -> {ms_preprocess, ms_sort, ms_blend, ms_wall}"""
    import torch
    score = torch.zeros(2 * n, dtype=torch.float32, device="cuda:0")
    sets = {"image_alone": (("image",), None), "depth_alpha": (("depth", "alpha"), None), "contribution": ((), score),
            "everything": (("image", "depth", "alpha"), score)}
    out = {}
    for name, (outputs, buf) in sets.items():
        call = lambda: ctx.render_aux(m["xyz"], m["cov6"], m["opacity"], m["color"], m["sh"].view(2 * n, 15, 3), 3, cam["viewmat"], cam["fx"], cam["fy"],
                                      cam["cx"], cam["cy"], width, height, (0.0, 0.0, 0.0), 3.0, outputs=outputs, contribution=buf)
        call()
        wall, parts = [], []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            parts.append(ctx.timing())
        out[name] = {"ms_" + k: statistics.median(p[k] for p in parts) for k in ("preprocess", "sort", "blend")}
        out[name]["ms_wall"] = statistics.median(wall)
    out["splats_that_counted"] = int((score > 0).sum())
    return out


def prune_case(model, h, repeats, cameras=8):
    """prune_unseen of the merged model over ``cameras`` 1280 x 720 views on a circle of radius 4 h around the box"""
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd.models.camera import Camera
    cams = []
    for k in range(cameras):
        ang = 2.0 * np.pi * k / cameras
        eye = 4.0 * h * np.array([np.sin(ang), 0.0, -np.cos(ang)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])               # world -> camera
        cams.append(Camera(R.T, -R @ eye, 1100.0, 1155.0, f"ring_{k}", 1280, 720))
    model.prune_unseen(cams)
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pruned, info = model.prune_unseen(cams)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return {"cameras": cameras, "ms_wall": statistics.median(wall), "n": info["n"], "n_kept": info["n_kept"]}


def run(n, width, height, focal, repeats, aux=False, prune=False):
    import torch
    from gaussiansplattingregistration_amd import raster, synth
    from gaussiansplattingregistration_amd.models.camera import Camera
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    a = synth.make_cloud_torch(n, seed=1, device="cuda:0", sh_degree=3)
    b = synth.apply_rigid_torch(a, synth.rigid_transform(5.0, (1, 1, 1), (0.1, -0.1, 0.05)))
    m = {k: torch.cat((a[k], b[k])).contiguous() for k in ("xyz", "cov6", "opacity", "color", "sh")}
    h = a["h"]
    del a, b
    cam = camera_on_the_z_axis(4.0 * h, width, height, focal)
    ctx = raster.context(0)
    call = lambda: ctx.render(m["xyz"], m["cov6"], m["opacity"], m["color"], m["sh"].view(2 * n, 15, 3), 3, cam["viewmat"], cam["fx"], cam["fy"], cam["cx"],
                              cam["cy"], width, height, (0.0, 0.0, 0.0), 3.0, with_stats=True)
    img, stats = call()
    torch.cuda.synchronize()
    wall, parts = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img, stats = call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(ctx.timing())
    med = lambda k: statistics.median(p[k] for p in parts)
    # the same image through the reference-named entry: GaussianModel -> get_full_covariance (n,3,3) -> the six entries again, per call
    model = GaussianModel("cuda:0").from_arrays(m["xyz"], m["color"], m["opacity"], m["cov6"], m["sh"], 3)
    c = Camera(cam["viewmat"][:3, :3].T, cam["viewmat"][:3, 3], cam["fx"], cam["fy"], "bench", width, height)
    rasterize_image(model, c, 1, (0.0, 0.0, 0.0), "cuda:0")
    named = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rasterize_image(model, c, 1, (0.0, 0.0, 0.0), "cuda:0")
        torch.cuda.synchronize()
        named.append((time.perf_counter() - t0) * 1e3)
    s = stats.cpu().tolist()
    ms = statistics.median(wall)
    extra = {}
    if aux:
        extra["aux"] = aux_cases(ctx, m, n, cam, width, height, repeats)
    if prune:
        extra["prune_unseen"] = prune_case(model, h, repeats)
    return {**extra, "splats": 2 * n, "width": width, "height": height, "ms_per_image_wall": ms, "ms_per_image_wall_rasterize_image": statistics.median(named), "ms_preprocess": med("preprocess"), "ms_sort": med("sort"),
            "ms_blend": med("blend"), "visible": s[0], "intersections": s[1], "nonempty_tiles": s[2], "splats_per_s": 2 * n / (ms * 1e-3),
            "intersections_per_s": s[1] / (ms * 1e-3), "finite": bool(torch.isfinite(img).all())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--splats", type=int, default=5_000_000, help="per cloud of the large pair")
    ap.add_argument("--small-only", action="store_true", help="the 2 x 1 M pair alone")
    ap.add_argument("--aux", action="store_true", help="also time render_aux per set of outputs, and prune_unseen over 8 cameras of the 2 x 1 M pair")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    cases = [run(1_000_000, 1280, 720, 1100.0, a.repeats, aux=a.aux, prune=a.aux)]
    if not a.small_only:
        cases.append(run(a.splats, 1920, 1080, 1650.0, a.repeats, aux=a.aux))
    print(json.dumps({"metric": "splat rasteriser, ms per image (median of %d)" % a.repeats, "cases": cases}))


if __name__ == "__main__":
    main()
