"""The fused L1 + D-SSIM loss kernel on the MI355X (``gsr_loss_l1_dssim``) at 1280 x 720 and 1920 x 1080:

* the call with and without the gradient, by events on the stream;
* the yardstick IN THE SAME RUN: the same loss written in torch on the device, forward plus backward -- float32 grouped ``conv2d`` over
  ``(1, 3, H, W)``, the formulation of ``utils.evaluation_utils.ssim``'s host branch, with autograd -- and its forward alone;
* one fine-tuning iteration (render, loss, backward, Adam on dc, sh_rest and opacity) with the ``l2`` loss and with ``l1_dssim`` on the
  scenes ``scripts/bench_raster_grad.py`` builds (2 x 1 M splats at 1280 x 720, 2 x 5 M at 1920 x 1080), wall clock.

    python scripts/bench_image_loss.py [--repeats 7] [--splats 5000000] [--small-only] [--no-finetune] [--out profiles/image_loss_bench.json]

Two warm-ups of every variant, then the variants alternate ``repeats`` times: medians, with the smallest and largest value beside them.
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


def torch_loss(image, target, window2d, lam):
    """(H, W, 3) float32 tensors -> the scalar loss, through five grouped conv2d calls"""
    import torch.nn.functional as Fn
    x, y = image.permute(2, 0, 1)[None], target.permute(2, 0, 1)[None]
    conv = lambda t: Fn.conv2d(t, window2d, padding=5, groups=3)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu12
    ssim = (((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))).mean()
    return (1 - lam) * (image - target).abs().mean() + lam * (1 - ssim)


def alternate(variants, repeats):
    """name -> callable; -> name -> [ms by stream events], after two warm-ups of each, the variants alternating"""
    import torch
    for _ in range(2):
        for call in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def run_loss(width, height, repeats, lam=0.2):
    import torch
    from gaussiansplattingregistration_amd import loss
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    image = torch.rand((height, width, 3), device="cuda:0", generator=gen)
    target = (image + 0.05 * torch.randn((height, width, 3), device="cuda:0", generator=gen)).clamp(0, 1)
    ctx = loss.context(0)
    parts = torch.empty(3, dtype=torch.float64, device="cuda:0")
    grad = torch.empty_like(image)
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).to(torch.float32).cuda()
    window2d = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    leaf = image.clone().requires_grad_(True)

    def torch_both():
        leaf.grad = None
        torch_loss(leaf, target, window2d, lam).backward()

    def torch_forward():
        with torch.no_grad():
            torch_loss(image, target, window2d, lam)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch_both()
    torch.cuda.synchronize()
    torch_peak = torch.cuda.max_memory_allocated() - base
    ms = alternate({"kernel_with_gradient": lambda: ctx.l1_dssim(image, target, lam, True, parts, grad),
                    "kernel_without_gradient": lambda: ctx.l1_dssim(image, target, lam, False, parts),
                    "torch_forward_backward": torch_both, "torch_forward": torch_forward}, repeats)
    torch_value = float(torch_loss(image, target, window2d, lam))
    torch_both()
    ctx.l1_dssim(image, target, lam, True, parts, grad)
    case = {"width": width, "height": height, "lambda": lam, "repeats": repeats, **{"ms_" + k: spread(v) for k, v in ms.items()},
            "loss_kernel": float(parts[0]), "loss_torch_float32": torch_value,
            "max_gradient_difference_over_max_gradient": float((grad - leaf.grad).abs().max() / grad.abs().max()),
            "torch_forward_backward_peak_temporary_bytes": int(torch_peak), "kernel_temporary_bytes": 16 * ((width + 15) // 16) * ((height + 15) // 16) + 16}
    case["torch_over_kernel_with_gradient"] = case["ms_torch_forward_backward"]["median"] / case["ms_kernel_with_gradient"]["median"]
    case["torch_over_kernel_without_gradient"] = case["ms_torch_forward"]["median"] / case["ms_kernel_without_gradient"]["median"]
    return case


def run_finetune(n, width, height, focal, repeats, lam=0.2):
    """the scene of scripts/bench_raster_grad.py; -> wall-clock ms of one iteration per loss, the two alternating"""
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import loss, raster, synth
    a = synth.make_cloud_torch(n, seed=1, device="cuda:0", sh_degree=3)
    b = synth.apply_rigid_torch(a, synth.rigid_transform(5.0, (1, 1, 1), (0.1, -0.1, 0.05)))
    m = {k: torch.cat((a[k], b[k])).contiguous() for k in ("xyz", "cov6", "opacity", "color", "sh")}
    h = a["h"]
    del a, b
    V = np.eye(4, dtype=np.float32)
    V[2, 3] = 4.0 * h
    cam = (V, float(focal), float(focal) * 1.05, width / 2.0, height / 2.0, width, height)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    target = torch.rand((height, width, 3), device="cuda:0", generator=gen)
    case = {"splats": 2 * n, "width": width, "height": height, "repeats": repeats}
    try:
        steps = {}
        for name in ("l2", "l1_dssim"):
            leaves = {k: m[k].clone().requires_grad_(True) for k in ("color", "sh", "opacity")}
            opt = torch.optim.Adam([{"params": [leaves["color"]], "lr": 2.5e-3}, {"params": [leaves["sh"]], "lr": 1.25e-4}, {"params": [leaves["opacity"]], "lr": 0.05}],
                                   eps=1e-15)

            def step(name=name, leaves=leaves, opt=opt):
                opt.zero_grad(set_to_none=True)
                image, _ = raster.render_differentiable(m["xyz"], m["cov6"], leaves["opacity"], leaves["color"], leaves["sh"].view(2 * n, 15, 3), 3, *cam)
                value = loss.l1_dssim(image, target, lam) if name == "l1_dssim" else ((image - target) ** 2).mean()
                value.backward()
                opt.step()
            steps[name] = step
        for _ in range(2):
            for step in steps.values():
                step()
        wall = {k: [] for k in steps}
        for _ in range(repeats):
            for k, step in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        case.update({"iteration_ms_wall_" + k: spread(v) for k, v in wall.items()})
        case["l1_dssim_over_l2"] = case["iteration_ms_wall_l1_dssim"]["median"] / case["iteration_ms_wall_l2"]["median"]
    except RuntimeError as e:
        case["error"] = str(e)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--splats", type=int, default=5_000_000, help="per cloud of the large pair of the fine-tuning iteration")
    ap.add_argument("--small-only", action="store_true", help="the fine-tuning iteration on the 2 x 1 M pair alone")
    ap.add_argument("--no-finetune", action="store_true", help="the loss alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_loss_bench.json"), help="the JSON is written here as well as printed")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    import torch
    result = {"metric": "gsr_loss_l1_dssim against the same loss in torch (float32 grouped conv2d, autograd), ms by stream events (median, min, max of %d "
                        "alternating repeats after 2 warm-ups); fine-tuning iterations by wall clock" % a.repeats,
              "loss": [run_loss(1280, 720, a.repeats), run_loss(1920, 1080, a.repeats)]}
    if not a.no_finetune:
        torch.cuda.empty_cache()
        result["finetune_iteration"] = [run_finetune(1_000_000, 1280, 720, 1100.0, a.repeats)]
        if not a.small_only:
            torch.cuda.empty_cache()
            result["finetune_iteration"].append(run_finetune(a.splats, 1920, 1080, 1650.0, a.repeats))
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
