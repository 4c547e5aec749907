"""The backward pass of the splat rasteriser on the MI355X: the two cases of DESIGN.md 14.5 -- the merged 2 x 1 M pair at
1280 x 720 and the merged 2 x 5 M pair at 1920 x 1080, SH degree 3 -- with ``gsr_raster_backward``'s four phases by device events
(preprocess + scan, emit + sort + ranges with the host wait, blend-backward, splat-backward), its wall clock, the bytes of the record
buffer (36 per intersection), and one fine-tuning iteration end to end (forward, loss, backward, Adam step on dc, sh_rest and opacity).

    python scripts/bench_raster_grad.py [--repeats 7] [--splats 5000000] [--small-only] [--out profiles/raster_grad_bench.json]

The yardstick is ``render_aux`` (image + alpha) of the same scene IN THE SAME RUN: after two warm-up calls of each, forward and backward
alternate ``repeats`` times; medians, with the smallest and largest value of every figure beside them.  A case that does not fit or
finish is reported with the library's message (which carries the intersection count), not shrunk.
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


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def run(n, width, height, focal, repeats):
    import torch
    from gaussiansplattingregistration_amd import raster, synth
    a = synth.make_cloud_torch(n, seed=1, device="cuda:0", sh_degree=3)
    b = synth.apply_rigid_torch(a, synth.rigid_transform(5.0, (1, 1, 1), (0.1, -0.1, 0.05)))
    m = {k: torch.cat((a[k], b[k])).contiguous() for k in ("xyz", "cov6", "opacity", "color", "sh")}
    h = a["h"]
    del a, b
    import numpy as np
    V = np.eye(4, dtype=np.float32)                                # a camera at (0, 0, -4 h) looking at the origin, as scripts/bench_raster.py
    V[2, 3] = 4.0 * h
    cam = dict(viewmat=V, fx=float(focal), fy=float(focal) * 1.05, cx=width / 2.0, cy=height / 2.0)
    ctx = raster.context(0)
    args = (m["xyz"], m["cov6"], m["opacity"], m["color"], m["sh"].view(2 * n, 15, 3), 3, cam["viewmat"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], width, height)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    g_img = torch.randn((height, width, 3), device="cuda:0", generator=gen)
    g_alpha = torch.randn((height, width), device="cuda:0", generator=gen)
    case = {"splats": 2 * n, "width": width, "height": height, "repeats": repeats}
    forward = lambda: ctx.render_aux(*args, (0.0, 0.0, 0.0), 3.0, outputs=("image", "alpha"), with_stats=True)
    backward = lambda: ctx.render_backward(*args, grad_image=g_img, grad_alpha=g_alpha, background=(0.0, 0.0, 0.0), radius_clip=3.0)
    try:
        for _ in range(2):
            stats = forward()["stats"]
            out = backward()
        torch.cuda.synchronize()
        fw_wall, bw_wall, fw_parts, bw_parts = [], [], [], []
        for _ in range(repeats):                                   # alternating: both see the same state of the machine
            for call, wall, parts, timing in ((forward, fw_wall, fw_parts, ctx.timing), (backward, bw_wall, bw_parts, ctx.backward_timing)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                parts.append(timing())
    except RuntimeError as e:
        case["error"] = str(e)
        return case
    s = stats.cpu().tolist()
    case.update(visible=s[0], intersections=s[1], nonempty_tiles=s[2], record_bytes=36 * s[1],
                forward_render_aux={"ms_wall": spread(fw_wall), **{"ms_" + k: spread([p[k] for p in fw_parts]) for k in ("preprocess", "sort", "blend")}},
                backward={"ms_wall": spread(bw_wall),
                          **{"ms_" + k: spread([p[k] for p in bw_parts]) for k in ("preprocess", "sort", "blend_backward", "splat_backward")}},
                finite=bool(all(torch.isfinite(v).all() for v in out.values())))
    case["backward_over_forward_wall"] = case["backward"]["ms_wall"]["median"] / case["forward_render_aux"]["ms_wall"]["median"]
    # one fine-tuning iteration end to end: forward, L2 loss against a fixed image, backward, Adam on dc, sh_rest, opacity
    try:
        leaves = {k: m[k].clone().requires_grad_(True) for k in ("color", "sh", "opacity")}
        opt = torch.optim.Adam([{"params": [leaves["color"]], "lr": 2.5e-3}, {"params": [leaves["sh"]], "lr": 1.25e-4}, {"params": [leaves["opacity"]], "lr": 0.05}],
                               eps=1e-15)
        target = torch.rand((height, width, 3), device="cuda:0", generator=gen)

        def step():
            opt.zero_grad(set_to_none=True)
            image, _ = raster.render_differentiable(m["xyz"], m["cov6"], leaves["opacity"], leaves["color"], leaves["sh"].view(2 * n, 15, 3), 3, *args[6:])
            loss = ((image - target) ** 2).mean()
            loss.backward()
            opt.step()
        for _ in range(2):
            step()
        it = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            it.append((time.perf_counter() - t0) * 1e3)
        case["finetune_iteration_ms_wall"] = spread(it)
    except RuntimeError as e:
        case["finetune_iteration_error"] = str(e)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--splats", type=int, default=5_000_000, help="per cloud of the large pair")
    ap.add_argument("--small-only", action="store_true", help="the 2 x 1 M pair alone")
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    cases = [run(1_000_000, 1280, 720, 1100.0, a.repeats)]
    if not a.small_only:
        import torch
        torch.cuda.empty_cache()
        cases.append(run(a.splats, 1920, 1080, 1650.0, a.repeats))
    result = {"metric": "gsr_raster_backward against render_aux of the same scene, ms (median, min, max of %d alternating repeats after 2 warm-ups)" % a.repeats,
              "cases": cases}
    text = json.dumps(result, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
