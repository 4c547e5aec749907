"""NumPy restatement of the rasteriser's auxiliary outputs: coverage, expected depth and the per-splat largest blending
weight, the model ``k_raster_blend_aux`` is held to.  Projection, alphas, the scene table and the fragility machinery are those of
``raster_model``; the pixel loop is restated here with ``D = sum z w`` next to the colour.

``render_aux(scene, cam, background, dtype)``: float64 by default, float32 with the kernel's operation order.  Its image is
``raster_model.render``'s bit for bit (tests/test_raster_aux_cpu.py).

The per-splat bounds (``contribution_bounds``).  Pixels are independent; on a NON-FRAGILE pixel (``raster_model``'s mask) every discrete
decision is robust, so a correct float32 implementation gives the model's weight ``w = alpha T`` there up to rounding; on a fragile one
it may decide otherwise, but whatever it decides, ``w <= alpha``.  With
  lo_i = the largest w_i over the non-fragile pixels,
  hi_i = the largest alpha_i (>= (1 - 1e-4) / 255) over the fragile pixels of the splat's tiles and of the ring of tiles around them
         (a fragile edge of the tile box moves it by one tile),
any correct implementation gives ``lo_i - tol <= contribution_i <= max(lo_i, hi_i) + tol``.  A splat is TIGHT when ``hi_i <= lo_i``.
A culled splat is not written at all, unless its cull itself is fragile (``cull_fragile``).
"""
from __future__ import annotations

import functools

import numpy as np

import raster_model as M

TILE = M.TILE


def render_aux(scene, cam, background=(0.0, 0.0, 0.0), dtype=np.float64, radius_clip=3.0):
    """-> dict(image (H,W,3), alpha (H,W), depth (H,W) in dtype; P: the projection; order: the visible splats front to back;
    per: splat -> (slice of its pixels, w there, alpha there))"""
    f = np.dtype(dtype).type
    P = M.project(scene, cam, dtype, radius_clip)
    W, H = P["W"], P["H"]
    vis = np.nonzero(P["ok"])[0]
    order = vis[np.lexsort((vis, P["z"][vis]))]
    img = np.zeros((H, W, 3), dtype)
    T = np.ones((H, W), dtype)
    D = np.zeros((H, W), dtype)
    done = np.zeros((H, W), bool)
    per = {}
    for i in order:
        xa, xb, ya, yb = P["x0"][i] * TILE, min(P["x1"][i] * TILE, W), P["y0"][i] * TILE, min(P["y1"][i] * TILE, H)
        xs, ys = np.arange(xa, xb), np.arange(ya, yb)
        sigma, alpha, _ = M._alpha(P, i, xs, ys, f)
        sl = (slice(ya, yb), slice(xa, xb))
        keep = ~done[sl] & ~(sigma < 0) & ~(alpha < f(1.0) / f(255.0))
        Tn = T[sl] * (f(1) - alpha)
        stop = keep & (Tn <= f(1e-4))
        upd = keep & ~stop
        w = np.where(upd, alpha * T[sl], f(0))
        for ch in range(3):
            img[sl + (ch,)] = img[sl + (ch,)] + P["rgb"][i, ch] * w
        D[sl] = D[sl] + P["z"][i] * w
        T[sl] = np.where(upd, Tn, T[sl])
        done[sl] |= stop
        per[int(i)] = (sl, w, alpha)
    bg = np.asarray(background, np.float32).astype(dtype)
    img = img + T[:, :, None] * bg[None, None, :]
    A = f(1) - T
    depth = D / np.maximum(A, f(1e-10))
    return dict(image=img, alpha=A, depth=depth, P=P, order=order, per=per)


def contribution_bounds(r64, fragile):
    """-> (lo, hi), two (n,) float64 arrays (zero for culled splats), from a float64 ``render_aux`` and ``raster_model``'s fragile mask"""
    P = r64["P"]
    n, W, H = len(P["ok"]), P["W"], P["H"]
    lo, hi = np.zeros(n), np.zeros(n)
    for i, (sl, w, _) in r64["per"].items():
        if w.size:
            lo[i] = float(np.where(fragile[sl], 0.0, w).max())
        xa, xb = max(P["x0"][i] - 1, 0) * TILE, min((P["x1"][i] + 1) * TILE, W)
        ya, yb = max(P["y0"][i] - 1, 0) * TILE, min((P["y1"][i] + 1) * TILE, H)
        fr = fragile[ya:yb, xa:xb]
        if fr.any():
            alpha = M._alpha(P, i, np.arange(xa, xb), np.arange(ya, yb), np.float64)[1]
            hi[i] = float(np.where(fr & (alpha >= M.ALPHA_FLOOR), alpha, 0.0).max())
    return lo, hi


def cull_fragile(P, radius_clip):
    """(n,) bool: the splats whose being culled or kept hangs on a decision within ``REL`` of its threshold -- the tests of
    ``raster_model._splat_fragility`` that concern the whole splat (depth range, determinant, the ceil that carries the radius clip, the
    image-bounds cull).  A model-culled splat that is not flagged is culled by every correct float32 implementation."""
    REL = M.REL
    z = P["z"]
    with np.errstate(all="ignore"):
        near_fr = (np.abs(z - M.NEAR) <= REL * M.NEAR) | (np.abs(z - M.FAR) <= REL * M.FAR)
        live = P["in_depth"] | near_fr
        det_fr = live & (np.abs(P["det"]) <= REL * np.abs(P["a"] * P["c"]))
        cand = live & (P["det"] > 0)
        r = P["r_real"]
        on_ceil = cand & (np.abs(r - np.round(r)) <= REL * r)
        ceil_fr = on_ceil & (np.round(r) <= radius_clip)               # the ceil decides the radius clip
        edge = np.zeros_like(cand)
        rad = P["rad"]
        for m, lim in ((P["mx"], P["W"]), (P["my"], P["H"])):
            for rr, who in ((rad, cand), (np.round(r), on_ceil), (np.round(r) + 1, on_ceil)):       # the radius itself may sit on a ceil
                tol = REL * (np.abs(m) + rr)
                edge |= who & ((np.abs(m + rr) <= tol) | (np.abs(m - rr - lim) <= tol))
        odd = live & ~np.isfinite(P["mx"] + P["my"] + rad)
    return near_fr | det_fr | ceil_fr | edge | odd


@functools.lru_cache(maxsize=None)
def scene_models(name):
    """Everything the tests need of a scene of ``raster_model.SCENES``, computed once and left unchanged: the scene, the camera, the
    background, ``raster_model.render`` in float64 (fragile mask), ``render_aux`` in both dtypes, and the bounds."""
    scene, cam, bg = M.build(name)
    s = M.scaled(scene)
    ref = M.render(s, cam, bg)
    r64, r32 = render_aux(s, cam, bg), render_aux(s, cam, bg, np.float32)
    lo, hi = contribution_bounds(r64, ref["fragile"])
    for a in (ref["image"], ref["fragile"], r64["image"], r64["alpha"], r64["depth"], r32["image"], r32["alpha"], r32["depth"], lo, hi):
        a.setflags(write=False)
    return dict(scene=scene, scaled=s, cam=cam, bg=bg, ref=ref, r64=r64, r32=r32, lo=lo, hi=hi)


def float32_cost(name):
    """what float32 costs the model itself on a scene: the largest float32-model versus float64-model difference of alpha (absolute,
    non-fragile pixels), of depth (relative to the depth, covered non-fragile pixels) and of contribution (absolute, tight splats)"""
    m = scene_models(name)
    nf = ~m["ref"]["fragile"]
    r64, r32 = m["r64"], m["r32"]
    covered = nf & (r64["alpha"] > 0)
    d_alpha = float(np.abs(r32["alpha"].astype(np.float64) - r64["alpha"])[nf].max())
    d_depth = float((np.abs(r32["depth"].astype(np.float64) - r64["depth"])[covered] / r64["depth"][covered]).max())
    vis = np.array(sorted(r64["per"]))
    tight = m["hi"][vis] <= m["lo"][vis]
    c32 = np.zeros(len(m["lo"]))
    for i, (sl, w, _) in r32["per"].items():
        if w.size:
            c32[i] = float(np.where(nf[sl], w, 0).max())
    d_contrib = float(np.abs(c32[vis] - m["lo"][vis])[tight].max())
    return {"alpha_max_abs_diff": d_alpha, "depth_max_rel_diff": d_depth, "contribution_max_abs_diff": d_contrib}


# ---- the scene with occluders of the pruning tests ---------------------------------------------------------------------------------
PRUNE_THRESHOLD, PRUNE_GUARD = 0.01, 1e-4
PRUNE_RADIUS_CLIP = 3.0          # the evaluation's clip, passed explicitly: the conditions of the scene (keep, drop, undecided) are stated for it
# (prune_models(0.0) is the same scene as prune_unseen's default sees it, without a clip: more rows are kept, the small splats count)
PRUNE_CAMS = (dict(M.CAM_A, width=128, height=96, focal=110.0), dict(M.CAM_B, width=120, height=90, focal=100.0))


def prune_scene():
    """``make_scene(1500, seed 31, sh_degree 1)`` whose first 40 splats are opaque discs (raw opacity 6, scales 0.15 .. 0.3) on the plane
    z = -1.5 +- 0.05, in x in [-1, 0.2] and y in [-1, 1]: between ``CAM_A`` and the left part of the box, beside ``CAM_B``."""
    scene = M.make_scene(n=1500, seed=31, sh_degree=1)
    rng = np.random.default_rng(32)
    m = 40
    scene["xyz"][:m] = np.column_stack([rng.uniform(-1.0, 0.2, m), rng.uniform(-1.0, 1.0, m), rng.uniform(-1.55, -1.45, m)]).astype(np.float32)
    scene["cov6"][:m] = M._cov6(rng, m, 0.15, 0.3)
    scene["opacity"][:m] = 6.0
    return scene


@functools.lru_cache(maxsize=None)
def prune_models(radius_clip=PRUNE_RADIUS_CLIP):
    """-> dict(scene, cams, lo, hi (maxima over both cameras, at ``radius_clip``), keep, drop: the rows decided at ``PRUNE_THRESHOLD`` with the
    guard band, fragile: the per-camera fragile fractions, refs: the float64 renders)"""
    scene = prune_scene()
    cams = [M.make_camera(**c) for c in PRUNE_CAMS]
    n = len(scene["xyz"])
    LO, HI = np.zeros(n), np.zeros(n)
    fragile, refs = [], []
    for cam in cams:
        ref = M.render(scene, cam, (0.0, 0.0, 0.0), radius_clip=radius_clip)
        r64 = render_aux(scene, cam, (0.0, 0.0, 0.0), radius_clip=radius_clip)
        lo, hi = contribution_bounds(r64, ref["fragile"])
        cf = cull_fragile(r64["P"], radius_clip) & ~r64["P"]["ok"]
        hi[cf] = 1.0                                   # a fragile cull: the row is undecided
        LO, HI = np.maximum(LO, lo), np.maximum(HI, hi)
        fragile.append(float(ref["fragile"].mean()))
        refs.append((ref, r64))
    keep = LO >= PRUNE_THRESHOLD + PRUNE_GUARD
    drop = np.maximum(LO, HI) < PRUNE_THRESHOLD - PRUNE_GUARD
    return dict(scene=scene, cams=cams, lo=LO, hi=HI, keep=keep, drop=drop, fragile=fragile, refs=refs)
