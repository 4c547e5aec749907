"""The covariance build kernels on the MI355X: ``gsr_cov_build`` and ``gsr_cov_build_backward`` at 1 M and 10 M splats, and
what tuning ``scaling`` / ``rotation`` adds to one fine-tuning iteration.

    python scripts/bench_cov_grad.py [--repeats 7] [--sizes 1000000 10000000] [--no-finetune] [--out profiles/covgrad_bench.json]

Per size, IN THE SAME RUN and alternating ``repeats`` times after two warm-up calls of each (medians, with the smallest and largest value
beside them):

  * the forward and the backward entry on CUDA tensors, by device events on torch's stream around the call and by the host clock around
    call + synchronise.  Both entries wait for the stream before they return (they are one-shot entries), so either figure holds one
    launch and one wait besides the kernel; ``gb_per_s`` is the bytes the kernel must move (forward 28 + 24, backward 52 + 28 per splat)
    over the event time, an END-TO-END rate of the call, not the kernel's share of peak;
  * a device-to-device copy that moves the same number of bytes (half of them read, half written), timed the same way;
  * the same function and its gradient as a plain torch chain under autograd (forward, then ``backward`` of ``sum(cov6 * g)``).

Then one fine-tuning iteration of the merged 2 x 1 M pair at 1280 x 720, SH degree 3 (the case of scripts/bench_raster_grad.py): forward,
L2 loss, backward, Adam step on ``(dc, sh_rest, opacity)`` against the same plus ``(scaling, rotation)``.  No target is set for any figure:
what is printed is what was measured.
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


def timed(call, torch):
    """-> (ms by device events around the call, ms by the host clock around call + synchronise)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def torch_chain(s, q):
    """the function as a plain torch chain: normalise, rotation matrix, L = R diag(exp s), L L^T, the six terms"""
    import torch
    u = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = u.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = R * torch.exp(s)[:, None, :]
    # (element-wise, not a batched matmul: one with more than 2^24 batches faults on some ROCm builds, and 10 M is close)
    return torch.stack([(L[:, i] * L[:, j]).sum(1) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1)


def run_size(n, repeats):
    import torch
    from gaussiansplattingregistration_amd import covariance
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    s = torch.empty((n, 3), device="cuda:0").uniform_(-6.0, 1.0, generator=gen)
    q = torch.randn((n, 4), device="cuda:0", generator=gen)
    g = torch.randn((n, 6), device="cuda:0", generator=gen)
    fwd_bytes, bwd_bytes = 52 * n, 80 * n
    src_f, dst_f = (torch.empty(fwd_bytes // 2, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    src_b, dst_b = (torch.empty(bwd_bytes // 2, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    sl, ql = s.clone().requires_grad_(True), q.clone().requires_grad_(True)

    def chain():
        sl.grad = ql.grad = None
        (torch_chain(sl, ql) * g).sum().backward()
    calls = {"forward": lambda: covariance.build_covariance(s, q), "backward": lambda: covariance.build_covariance_backward(s, q, g),
             "copy_forward_bytes": lambda: dst_f.copy_(src_f), "copy_backward_bytes": lambda: dst_b.copy_(src_b), "torch_chain_forward_and_backward": chain}
    case = {"splats": n, "repeats": repeats, "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes}
    try:
        for _ in range(2):
            for call in calls.values():
                call()
        torch.cuda.synchronize()
        ev, wall = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(repeats):                                   # alternating: all see the same state of the machine
            for k, call in calls.items():
                e, w = timed(call, torch)
                ev[k].append(e)
                wall[k].append(w)
    except RuntimeError as e:
        case["error"] = str(e)
        return case
    for k in calls:
        case[k] = {"ms_events": spread(ev[k]), "ms_wall": spread(wall[k])}
    for k, nbytes in (("forward", fwd_bytes), ("backward", bwd_bytes), ("copy_forward_bytes", fwd_bytes), ("copy_backward_bytes", bwd_bytes)):
        case[k]["gb_per_s"] = nbytes / (case[k]["ms_events"]["median"] * 1e-3) / 1e9
    both = case["forward"]["ms_events"]["median"] + case["backward"]["ms_events"]["median"]
    case["torch_chain_over_kernels"] = case["torch_chain_forward_and_backward"]["ms_events"]["median"] / both
    # the kernels against the chain on these inputs (float32 both; not a test, a plausibility figure for the timing)
    want = torch_chain(sl, ql)
    got = covariance.build_covariance(s, q)
    case["max_abs_difference_to_torch_chain"] = float((got - want).abs().max())
    return case


def run_finetune(n, width, height, focal, repeats):
    import numpy as np
    import torch
    from gaussiansplattingregistration_amd import _lib, covariance, raster, synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    a = synth.make_cloud_torch(n, seed=1, device="cuda:0", sh_degree=3)
    b = synth.apply_rigid_torch(a, synth.rigid_transform(5.0, (1, 1, 1), (0.1, -0.1, 0.05)))
    m = {k: torch.cat((a[k], b[k])).contiguous() for k in ("xyz", "cov6", "opacity", "color", "sh")}
    h = a["h"]
    del a, b
    holder = GaussianModel("cuda:0")
    holder._covariance = m["cov6"]
    scaling, rotation, _ = holder._decompose(_lib.GSR_DECOMP_EXACT)
    V = np.eye(4, dtype=np.float32)                                # a camera at (0, 0, -4 h) looking at the origin, as scripts/bench_raster_grad.py
    V[2, 3] = 4.0 * h
    cam = (V, float(focal), float(focal) * 1.05, width / 2.0, height / 2.0, width, height)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    target = torch.rand((height, width, 3), device="cuda:0", generator=gen)
    case = {"splats": 2 * n, "width": width, "height": height, "repeats": repeats}

    def variant(with_geometry):
        leaves = {k: m[k].clone().requires_grad_(True) for k in ("color", "sh", "opacity")}
        groups = [{"params": [leaves["color"]], "lr": 2.5e-3}, {"params": [leaves["sh"]], "lr": 1.25e-4}, {"params": [leaves["opacity"]], "lr": 0.05}]
        if with_geometry:
            leaves["scaling"], leaves["rotation"] = scaling.clone().requires_grad_(True), rotation.clone().requires_grad_(True)
            groups += [{"params": [leaves["scaling"]], "lr": 5e-3}, {"params": [leaves["rotation"]], "lr": 1e-3}]
        opt = torch.optim.Adam(groups, eps=1e-15)

        def step():
            opt.zero_grad(set_to_none=True)
            cov = covariance.covariance_from_scale_rotation(leaves["scaling"], leaves["rotation"]) if with_geometry else m["cov6"]
            image, _ = raster.render_differentiable(m["xyz"], cov, leaves["opacity"], leaves["color"], leaves["sh"].view(2 * n, 15, 3), 3, *cam)
            loss = ((image - target) ** 2).mean()
            loss.backward()
            opt.step()
        return step
    try:
        steps = {"dc_sh_rest_opacity": variant(False), "plus_scaling_rotation": variant(True)}
        for _ in range(2):
            for step in steps.values():
                step()
        torch.cuda.synchronize()
        wall = {k: [] for k in steps}
        for _ in range(repeats):
            for k, step in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        for k in steps:
            case[k] = {"iteration_ms_wall": spread(wall[k])}
        case["added_ms_median"] = case["plus_scaling_rotation"]["iteration_ms_wall"]["median"] - case["dc_sh_rest_opacity"]["iteration_ms_wall"]["median"]
    except RuntimeError as e:
        case["error"] = str(e)
    return case


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--no-finetune", action="store_true", help="the kernels alone")
    ap.add_argument("--finetune-splats", type=int, default=1_000_000, help="per cloud of the merged pair")
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_hip()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cov_grad.py measures on the GPU: no device is visible")
    result = {"metric": "gsr_cov_build / gsr_cov_build_backward, ms (median, min, max of %d alternating repeats after 2 warm-ups)" % a.repeats,
              "kernels": [run_size(n, a.repeats) for n in a.sizes]}
    if not a.no_finetune:
        torch.cuda.empty_cache()
        result["finetune_iteration"] = run_finetune(a.finetune_splats, 1280, 720, 1100.0, a.repeats)
    text = json.dumps(result, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
