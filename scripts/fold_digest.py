"""sha256 of the raw bytes of every float64 sum that passes through the fixed-order fold (csrc/gsr_fold.h), on seeded inputs, by the
Python entry points alone: ICP sums of every estimator and loss, the information matrix, ICP registrations, the mixture-to-mixture
sums and registration, the colour sums, the photometric sums and the FGR optimisation.  Two builds that fold in the same order write
the same file; run it from a checkout of either commit (or with GSR_HIP_LIB where the library has the checkout's symbols).

    python scripts/fold_digest.py OUT.json

Clouds of 1, 255, 257 and 70 000 points (the last: more than 64 blocks, the grid-stride kernels), images of 16 x 16 and 250 x 130.
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
CLOUDS = (1, 255, 257, 70000)
IMAGES = ((16, 16), (250, 130))          # width, height


def sha(*values):
    h = hashlib.sha256()
    for v in values:
        h.update(np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tobytes())
    return h.hexdigest()


def record(out, name, fn):
    try:
        out[name] = fn()
    except Exception as e:          # the message names the entry point and the reason, no addresses
        out[name] = "raised: " + str(e)


def spd6(rng, n, size):
    L = rng.normal(size=(n, 3, 3)) * size
    Cm = L @ np.transpose(L, (0, 2, 1)) + (0.05 * size) ** 2 * np.eye(3)
    return np.stack([Cm[:, 0, 0], Cm[:, 0, 1], Cm[:, 0, 2], Cm[:, 1, 1], Cm[:, 1, 2], Cm[:, 2, 2]], -1)


def cloud_case(out, n):
    from gaussiansplattingregistration_amd import d2d, features, harmonize, icp, synth
    rng = np.random.default_rng(1000 + n)
    spacing = n ** (-1.0 / 3.0)
    mc = min(0.5, 2.0 * spacing)
    tx = rng.random((n, 3)).astype(np.float32)
    T = synth.rigid_transform(3.0, (0.3, 1.0, -0.5), 0.2 * spacing * np.array([1.0, -0.5, 0.25]))
    sx = ((tx.astype(np.float64) + rng.normal(size=(n, 3)) * 0.05 * spacing - T[:3, 3]) @ T[:3, :3]).astype(np.float32)    # T sx ~ tx
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tcov, scov = spd6(rng, n, 0.5 * spacing), spd6(rng, n, 0.5 * spacing)
    trgb, srgb = rng.random((n, 3)), rng.random((n, 3))
    with icp.IcpContext(device=0) as ctx:
        ctx.set_target(tx, nrm, mc)
        ctx.set_source(sx)
        ctx.set_target_cov(tcov)
        ctx.set_source_cov(scov)
        ctx.set_target_color(trgb)
        ctx.set_source_color(srgb)
        for kind in range(5):
            for loss in range(5):
                record(out, f"icp.accumulate n={n} kind={kind} loss={loss}", lambda: sha(ctx.accumulate(T, kind, loss, 0.1)))
            def reg():
                r = ctx.register(T, kind=kind, max_iter=8)
                return sha(r["transformation"], r["fitness"], r["inlier_rmse"], r["iterations"])
            record(out, f"icp.register n={n} kind={kind}", reg)
        record(out, f"icp.information n={n}", lambda: sha(*ctx.information(T)))
    with d2d.D2DContext(0) as dctx:
        dctx.set_target(tx, tcov.astype(np.float32), None, mc)
        dctx.set_source(sx, scov.astype(np.float32), None)
        record(out, f"d2d.accumulate n={n}", lambda: sha(dctx.accumulate(T, 1.25, 1e-5)))
        def dreg():
            r = dctx.register(T, 1.25, 1e-5, max_iteration=5)
            return sha(r["transformation"], r["score"], r["fitness"], r["mahalanobis_rmse"], r["iterations"], r["n_pairs"], r["n_singular"])
        record(out, f"d2d.register n={n}", dreg)
    dc_s, dc_t = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    op_s, op_t = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    pairs = np.stack([rng.permutation(n), np.arange(n)], 1).astype(np.int32)
    P = harmonize.IDENTITY + rng.uniform(-0.1, 0.1, (3, 4))
    record(out, f"harmonize.color_sums n={n}", lambda: sha(harmonize.color_sums(dc_s, op_s, dc_t, op_t, pairs, P_s=P, huber=0.1)[0]))
    corres = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    def fgr():
        r = features.fgr_optimize(sx, tx, corres, maximum_correspondence_distance=mc)
        return sha(r["transformation"], r["n_corres"], r["iterations"], r["scale_global"])
    record(out, f"features.fgr_optimize n={n}", fgr)


def image_case(out, width, height):
    from gaussiansplattingregistration_amd import photo
    from gaussiansplattingregistration_amd.params import PhotometricParams
    rng = np.random.default_rng(width)
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")

    def maps(k):
        img = np.stack([0.5 + 0.3 * np.sin(0.03 * x + 0.02 * y + c + 0.05 * k) for c in range(3)], -1) + 0.02 * rng.normal(size=(height, width, 3))
        depth = 2.0 + 0.3 * np.sin(0.021 * x + 0.4) * np.cos(0.017 * y) + 0.05 * k * rng.random((height, width))
        alpha = np.where(rng.random((height, width)) < 0.02, 0.1, 0.9)
        return dict(image=np.ascontiguousarray(img, np.float32), depth=np.ascontiguousarray(depth, np.float32), alpha=np.ascontiguousarray(alpha, np.float32))
    src, tgt = maps(0), maps(1)
    V = np.eye(4)
    V[2, 3] = 2.5
    cam = photo.PhotoCamera(V, 1.1 * width, 1.1 * width, width / 2, height / 2, width, height)
    record(out, f"photo.accumulate_sums {width}x{height}", lambda: sha(photo.accumulate_sums(src, tgt, cam, PhotometricParams(max_depth_diff=0.25), device=0)))


def main():
    import __graft_entry__ as g
    g.build_hip()
    out = {}
    for n in CLOUDS:
        cloud_case(out, n)
    for w, h in IMAGES:
        image_case(out, w, h)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    raised = sum(1 for v in out.values() if v.startswith("raised"))
    print("wrote %s: %d entries, %d of them refusals" % (sys.argv[1], len(out), raised))


if __name__ == "__main__":
    main()
