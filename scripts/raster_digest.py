"""sha256 of the raw bytes of every output of the rasteriser's three entries (csrc/raster.hip), by the Python entry points alone:
``render`` with stats, ``render_aux`` in four forms (every output plus a contribution buffer; depth + alpha; the contribution alone;
the image alone) and ``render_backward`` with all five gradients in three forms (both upstream gradients, grad_image alone, grad_alpha
alone).  Two builds that compute the same bits write the same file; run it from a checkout of either commit.

    python scripts/raster_digest.py OUT.json

Scenes: the six of tests/raster_model.SCENES and raster_grad_model's grad_edges; an empty model; a 1 x 1 and a 17 x 17 image; and a
16 x 16 image whose single tile holds exactly 255, 256 and 257 intersections (small faint splats stacked at increasing depth, as rows
9 .. 308 of grad_edges: an LDS batch one short, exactly full, and a second batch of one -- the stats entry shows the count).
A call that raises is recorded with its message: both builds must refuse alike.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def record(out, name, fn):
    try:
        for k, v in fn().items():
            out[name + " -> " + k] = sha(v) if k != "stats" else "stats %s %s" % (v.cpu().tolist(), sha(v))
    except Exception as e:          # the message names the entry point and the reason, no addresses
        out[name] = "raised: " + str(e)


def stack_scene(k):
    """k faint splats of 0.075 world units inside the one tile of a 16 x 16 image, every one at a depth of its own"""
    import raster_model as M
    rng = np.random.default_rng(2800 + k)
    W = H = 16
    f = 40.0
    z = np.linspace(-0.5, 0.4, k)
    u, v = rng.uniform(5.5, 10.5, k), rng.uniform(5.5, 10.5, k)
    xyz = np.stack([-(u - W / 2.0) * (z + 3.0) / f, -(v - H / 2.0) * (z + 3.0) / (1.05 * f), z], -1)
    s2 = 0.075 ** 2
    scene = dict(xyz=xyz.astype(np.float32), cov6=np.tile(np.float32([s2, 0, 0, s2, 0, s2]), (k, 1)), opacity=rng.uniform(-4.2, -3.6, k).astype(np.float32),
                 color=((rng.uniform(0.25, 0.75, (k, 3)) - 0.5) / M.C0).astype(np.float32), sh=rng.normal(0, 0.02, (k, 9)).astype(np.float32), sh_degree=1)
    return scene, M.make_camera(eye=(0.0, 0.0, -3.0), target=(0.0, 0.0, 0.0), width=W, height=H, focal=f), (0.3, 0.6, 0.1)


def cases():
    import raster_grad_model as G
    import raster_model as M
    for name in list(M.SCENES) + [G.GRAD_EDGES]:
        yield (name,) + G.build(name)
    scene, _, bg = G.build("giants_tiny")          # its giants cover any image, its cluster of small splats sits near the centre
    yield "empty", {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in scene.items()}, M.make_camera(**G.EDGE_CAM), bg
    yield "image_1x1", scene, M.make_camera(**dict(M.CAM_A, width=1, height=1, focal=20.0)), bg
    yield "image_17x17", scene, M.make_camera(**dict(M.CAM_A, width=17, height=17, focal=40.0)), bg
    for k in (255, 256, 257):
        yield ("stack_%d" % k,) + stack_scene(k)


def digest_case(out, ctx, name, scene, cam, bg):
    import raster_grad_model as G
    import torch
    n, K = scene["xyz"].shape[0], (scene["sh_degree"] + 1) ** 2 - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    args = (dev(scene["xyz"]), dev(scene["cov6"]), dev(scene["opacity"]), dev(scene["color"]), dev(scene["sh"]).reshape(n, K, 3) if K else None,
            scene["sh_degree"], cam["viewmat"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])
    H, W = cam["height"], cam["width"]

    def render():
        image, stats = ctx.render(*args, background=bg, with_stats=True)
        return {"image": image, "stats": stats}
    record(out, name + ": render", render)
    score = lambda: torch.zeros(n, dtype=torch.float32, device="cuda")
    for form, outputs, buf in (("everything", ("image", "depth", "alpha"), score()), ("depth+alpha", ("depth", "alpha"), None),
                               ("contribution alone", (), score()), ("image alone", ("image",), None)):
        record(out, name + ": render_aux " + form, lambda: ctx.render_aux(*args, background=bg, outputs=outputs, contribution=buf, with_stats=True))
    g_c, g_a = (dev(g) for g in G.upstream(name, H, W))
    for form, kw in (("both", dict(grad_image=g_c, grad_alpha=g_a)), ("grad_image alone", dict(grad_image=g_c)), ("grad_alpha alone", dict(grad_alpha=g_a))):
        record(out, name + ": render_backward " + form, lambda: ctx.render_backward(*args, background=bg, with_stats=True, **kw))


def main():
    import __graft_entry__ as g
    g.build_hip()
    from gaussiansplattingregistration_amd import raster
    out = {}
    ctx = raster.context(0)
    for case in cases():
        digest_case(out, ctx, *case)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    raised = sum(1 for v in out.values() if v.startswith("raised"))
    print("wrote %s: %d entries, %d of them refusals" % (sys.argv[1], len(out), raised))
    for k in sorted(out):
        if k.endswith("render -> stats"):
            print(k, out[k].rsplit(" ", 1)[0])


if __name__ == "__main__":
    main()
