"""NumPy restatement of the rasteriser's semantics and of the image metrics, the model csrc/raster.hip is held to.

``render(scene, cam, background, dtype)`` loops over the depth-sorted visible splats and blends every pixel of the tiles each one
touches (no binning, no sort keys): float64 by default, float32 with the kernel's operation order when ``dtype=np.float32``.  In
float64 it also returns the per-pixel FRAGILE mask: pixels on which some discrete decision of a splat sits within a relative
``REL`` = 1e-4 of its threshold, so that float32 may legitimately decide otherwise -- near and far plane, ``det <= 0``, the ``ceil`` of the
radius (which carries ``radius <= clip``), the image-bounds cull, the edges of the tile box, ``sigma < 0``, ``alpha < 1/255``,
``T (1 - alpha) <= 1e-4`` and a depth order float32 does not reproduce -- and ``fragile_alpha``: the sum of the alphas of the splats
flagged on each pixel, the most such a decision can move it when colours stay within [0, 1].

``scene``: dict(xyz (n,3), cov6 (n,6), opacity (n,) raw, color (n,3) SH DC, sh (n,3K) coefficient-major, sh_degree).
``cam``: dict(viewmat (4,4), fx, fy, cx, cy, width, height).
"""
from __future__ import annotations

import numpy as np

TILE = 16
REL = 1e-4
ALPHA_FLOOR = (1.0 - REL) / 255.0
NEAR, FAR, EPS2D = 0.01, 1e10, 0.3
C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277, -0.5900435899266435)


def sh_basis(degree, d):
    """(n, (degree+1)^2 - 1) rest basis of 3DGS along the unit vectors d (n,3), in d's dtype"""
    f = d.dtype.type
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    cols = []
    if degree > 0:
        cols += [f(-C1) * y, f(C1) * z, f(-C1) * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        cols += [f(C2[0]) * xy, f(C2[1]) * yz, f(C2[2]) * (f(2) * zz - xx - yy), f(C2[3]) * xz, f(C2[4]) * (xx - yy)]
    if degree > 2:
        cols += [f(C3[0]) * y * (f(3) * xx - yy), f(C3[1]) * xy * z, f(C3[2]) * y * (f(4) * zz - xx - yy),
                 f(C3[3]) * z * (f(2) * zz - f(3) * xx - f(3) * yy), f(C3[4]) * x * (f(4) * zz - xx - yy), f(C3[5]) * z * (xx - yy),
                 f(C3[6]) * x * (xx - f(3) * yy)]
    return np.stack(cols, 1) if cols else np.zeros((d.shape[0], 0), d.dtype)


def project(scene, cam, dtype=np.float64, radius_clip=3.0):
    """Everything the preprocessing kernel computes, for all splats at once, in ``dtype`` with the kernel's operation order."""
    f = np.dtype(dtype).type
    V = np.asarray(cam["viewmat"], np.float32).reshape(4, 4)
    R, t = V[:3, :3].astype(dtype), V[:3, 3].astype(dtype)
    campos = (-(V[:3, :3].astype(np.float64).T @ V[:3, 3].astype(np.float64))).astype(np.float32).astype(dtype)
    W, H = int(cam["width"]), int(cam["height"])
    fx, fy, cx, cy = (f(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    p = np.asarray(scene["xyz"], np.float32).astype(dtype)
    c6 = np.asarray(scene["cov6"], np.float32).astype(dtype)
    n = p.shape[0]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    pc = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
    pz = pc[2]
    S = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
    M = [[(R[r, 0] * S[0][q] + R[r, 1] * S[1][q]) + R[r, 2] * S[2][q] for q in range(3)] for r in range(3)]
    Sc = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for q in range(r, 3):
            Sc[r][q] = Sc[q][r] = (M[r][0] * R[q, 0] + M[r][1] * R[q, 1]) + M[r][2] * R[q, 2]
    tan_x, tan_y = f(0.5) * f(W) / fx, f(0.5) * f(H) / fy
    lim_xp, lim_xn = (f(W) - cx) / fx + f(0.3) * tan_x, cx / fx + f(0.3) * tan_x
    lim_yp, lim_yn = (f(H) - cy) / fy + f(0.3) * tan_y, cy / fy + f(0.3) * tan_y
    with np.errstate(all="ignore"):
        rz = f(1) / pz
        tx = pz * np.minimum(lim_xp, np.maximum(-lim_xn, pc[0] * rz))
        ty = pz * np.minimum(lim_yp, np.maximum(-lim_yn, pc[1] * rz))
        rz2 = rz * rz
        j00, j02, j11, j12 = fx * rz, -(fx * tx) * rz2, fy * rz, -(fy * ty) * rz2
        v00, v01, v02 = Sc[0][0] * j00 + Sc[0][2] * j02, Sc[1][0] * j00 + Sc[1][2] * j02, Sc[2][0] * j00 + Sc[2][2] * j02
        v11, v12 = Sc[1][1] * j11 + Sc[1][2] * j12, Sc[2][1] * j11 + Sc[2][2] * j12
        a = (j00 * v00 + j02 * v02) + f(EPS2D)
        b = j11 * v01 + j12 * v02
        c = (j11 * v11 + j12 * v12) + f(EPS2D)
        det = a * c - b * b
        mx, my = (fx * pc[0]) * rz + cx, (fy * pc[1]) * rz + cy
        bm = f(0.5) * (a + c)
        r_real = f(3) * np.sqrt(bm + np.sqrt(np.maximum(f(0.01), bm * bm - det)))
        rad = np.ceil(r_real)
        in_depth = (pz >= f(NEAR)) & (pz <= f(FAR))
        ok = in_depth & (det > 0) & (rad > f(radius_clip))
        ok &= ~((mx + rad <= 0) | (mx - rad >= f(W)) | (my + rad <= 0) | (my - rad >= f(H)))
        tiles_x, tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        inv = f(1.0 / TILE)

        def box(m, r, nt):
            lo = np.clip(np.floor(np.where(ok, (m - r) * inv, 0)), 0, nt).astype(np.int64)
            hi = np.clip(np.ceil(np.where(ok, (m + r) * inv, 0)), 0, nt).astype(np.int64)
            return lo, hi
        x0, x1 = box(mx, rad, tiles_x)
        y0, y1 = box(my, rad, tiles_y)
        touched = np.where(ok, (x1 - x0) * (y1 - y0), 0)
        ok &= touched > 0
        d = p - campos
        d = d * (f(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))[:, None]
        deg = int(scene["sh_degree"])
        basis = sh_basis(deg, d)
        dc = np.asarray(scene["color"], np.float32).astype(dtype)
        rest = np.asarray(scene["sh"], np.float32).astype(dtype).reshape(n, -1, 3)
        rgb = f(C0) * dc
        for k in range(basis.shape[1]):
            rgb = rgb + basis[:, k:k + 1] * rest[:, k, :]
        rgb = np.maximum(rgb + f(0.5), f(0))
        op = f(1) / (f(1) + np.exp(-np.asarray(scene["opacity"], np.float32).astype(dtype).reshape(n)))
        conic = np.stack([c / det, -b / det, a / det], 1)
    return dict(ok=ok, z=pz, mx=mx, my=my, a=a, b=b, c=c, det=det, r_real=r_real, rad=rad, x0=x0, x1=x1, y0=y0, y1=y1, touched=touched, rgb=rgb, op=op,
                conic=conic, in_depth=in_depth, W=W, H=H, tiles_x=tiles_x, tiles_y=tiles_y)


def _alpha(P, i, xs, ys, f):
    """(sigma, alpha, magnitude of sigma's terms) of splat i on the pixel grid ys x xs"""
    dx = (P["mx"][i] - (xs.astype(P["mx"].dtype) + f(0.5)))[None, :]
    dy = (P["my"][i] - (ys.astype(P["mx"].dtype) + f(0.5)))[:, None]
    A, B, C = P["conic"][i]
    sigma = f(0.5) * (A * dx * dx + C * dy * dy) + B * dx * dy
    mag = f(0.5) * (abs(A) * dx * dx + abs(C) * dy * dy) + abs(B * dx * dy)
    with np.errstate(over="ignore"):
        alpha = np.minimum(f(0.999), P["op"][i] * np.exp(-sigma))
    return sigma, alpha, mag


def render(scene, cam, background=(0.0, 0.0, 0.0), dtype=np.float64, radius_clip=3.0):
    """-> dict(image (H,W,3) in dtype, visible, intersections, nonempty_tiles[, fragile (H,W) bool, fragile_alpha (H,W)] in float64 mode,
    max_rgb: the largest splat colour among the visible ones)"""
    f = np.dtype(dtype).type
    P = project(scene, cam, dtype, radius_clip)
    W, H = P["W"], P["H"]
    vis = np.nonzero(P["ok"])[0]
    z32 = project(scene, cam, np.float32, radius_clip)["z"] if dtype == np.float64 else P["z"]
    order = vis[np.lexsort((vis, P["z"][vis]))]
    img = np.zeros((H, W, 3), dtype)
    T = np.ones((H, W), dtype)
    done = np.zeros((H, W), bool)
    track = dtype == np.float64
    fragile = np.zeros((H, W), bool)
    fal = np.zeros((H, W), np.float64)
    tiles = set()
    for i in order:
        xa, xb, ya, yb = P["x0"][i] * TILE, min(P["x1"][i] * TILE, W), P["y0"][i] * TILE, min(P["y1"][i] * TILE, H)
        for ty in range(P["y0"][i], P["y1"][i]):
            tiles.update(ty * P["tiles_x"] + tx for tx in range(P["x0"][i], P["x1"][i]))
        xs, ys = np.arange(xa, xb), np.arange(ya, yb)
        sigma, alpha, mag = _alpha(P, i, xs, ys, f)
        sl = (slice(ya, yb), slice(xa, xb))
        alive = ~done[sl]
        keep = alive & ~(sigma < 0) & ~(alpha < f(1.0) / f(255.0))
        Tn = T[sl] * (f(1) - alpha)
        stop = keep & (Tn <= f(1e-4))
        upd = keep & ~stop
        if track:
            fr = alive & ((np.abs(sigma) <= REL * mag) | (np.abs(alpha - 1.0 / 255.0) <= REL / 255.0) | (keep & (np.abs(Tn - 1e-4) <= REL * 1e-4)))
            fragile[sl] |= fr
            fal[sl] += np.where(fr, alpha, 0.0)
        w = np.where(upd, alpha * T[sl], f(0))
        for ch in range(3):
            img[sl + (ch,)] = img[sl + (ch,)] + P["rgb"][i, ch] * w
        T[sl] = np.where(upd, Tn, T[sl])
        done[sl] |= stop
    bg = np.asarray(background, np.float32).astype(dtype)
    img = img + T[:, :, None] * bg[None, None, :]
    out = dict(image=img, visible=int(vis.size), intersections=int(P["touched"][vis].sum()), nonempty_tiles=len(tiles),
               max_rgb=float(P["rgb"][vis].max()) if vis.size else 0.0)
    if track:
        _splat_fragility(P, z32, order, radius_clip, fragile, fal)
        out.update(fragile=fragile, fragile_alpha=fal)
    return out


def _flag_box(P, i, rad, fragile, fal, whole=False, outside=None):
    """flag the pixels of the tiles the box of radius ``rad`` (+ one tile on every side) covers on which the splat would count, and
    add its alpha there.  ``outside``: only pixels not strictly inside the box of that radius around the mean -- a decision that
    moves an edge of the tile box by one tile changes nothing inside the radius box, which every candidate tile box contains."""
    W, H = P["W"], P["H"]
    if whole or not np.isfinite(P["mx"][i] + P["my"][i] + rad):
        fragile[:] = True
        fal += 1.0
        return
    xa = int(np.clip((np.floor((P["mx"][i] - rad) / TILE) - 1) * TILE, 0, W)); xb = int(np.clip((np.ceil((P["mx"][i] + rad) / TILE) + 1) * TILE, 0, W))
    ya = int(np.clip((np.floor((P["my"][i] - rad) / TILE) - 1) * TILE, 0, H)); yb = int(np.clip((np.ceil((P["my"][i] + rad) / TILE) + 1) * TILE, 0, H))
    if xa >= xb or ya >= yb:
        return
    alpha = np.nan_to_num(_alpha(P, i, np.arange(xa, xb), np.arange(ya, yb), np.float64)[1], nan=1.0)
    hit = alpha >= ALPHA_FLOOR                        # below 1/255 the splat is skipped on that pixel whether it is kept or culled
    if outside is not None:
        dx = np.abs(P["mx"][i] - (np.arange(xa, xb) + 0.5))[None, :]
        dy = np.abs(P["my"][i] - (np.arange(ya, yb) + 0.5))[:, None]
        hit &= (dx >= outside) | (dy >= outside)
    fragile[ya:yb, xa:xb] |= hit
    fal[ya:yb, xa:xb] += np.where(hit, alpha, 0.0)


def _splat_fragility(P, z32, order, radius_clip, fragile, fal):
    """the per-splat decisions (float64 values against their thresholds) and the depth order float32 gives"""
    W, H = P["W"], P["H"]
    z = P["z"]
    near_fr = (np.abs(z - NEAR) <= REL * NEAR) | (np.abs(z - FAR) <= REL * FAR)          # either end of the depth range
    live = P["in_depth"] | near_fr
    det_fr = live & (np.abs(P["det"]) <= REL * np.abs(P["a"] * P["c"]))
    for i in np.nonzero(near_fr | det_fr)[0]:
        _flag_box(P, i, 0.0, fragile, fal, whole=True)
    cand = live & (P["det"] > 0) & ~near_fr & ~det_fr
    r = P["r_real"]
    ceil_fr = cand & (np.abs(r - np.round(r)) <= REL * r)
    rad = P["rad"]
    mx, my = P["mx"], P["my"]
    big = cand & (rad > radius_clip)
    edge = np.zeros_like(cand)
    for m, lim in ((mx, W), (my, H)):
        tol = REL * (np.abs(m) + rad)
        edge |= big & ((np.abs(m + rad) <= tol) | (np.abs(m - rad - lim) <= tol))              # the image-bounds cull
        for v in (m - rad, m + rad):                                                           # the edges of the tile box
            edge |= big & (np.abs(v - np.round(v / TILE) * TILE) <= tol)
    with np.errstate(invalid="ignore"):
        for i in np.nonzero(ceil_fr | edge)[0]:
            # the whole splat is at stake only where the ceil decides the radius clip; otherwise one ring of tiles is
            whole_splat = ceil_fr[i] and np.round(r[i]) <= radius_clip
            _flag_box(P, i, rad[i] + (1.0 if ceil_fr[i] else 0.0), fragile, fal, outside=None if whole_splat else np.round(r[i]) - 1.0)
    # depth order: a pair float32 does not order strictly the same way
    for k in (1, 2, 3):
        for i, j in zip(order[:-k], order[k:]):
            if not z32[i] < z32[j]:
                xa, xb = max(P["x0"][i], P["x0"][j]) * TILE, min(min(P["x1"][i], P["x1"][j]) * TILE, W)
                ya, yb = max(P["y0"][i], P["y0"][j]) * TILE, min(min(P["y1"][i], P["y1"][j]) * TILE, H)
                if xa < xb and ya < yb:
                    al = [_alpha(P, s, np.arange(xa, xb), np.arange(ya, yb), np.float64)[1] for s in (i, j)]
                    hit = (al[0] >= ALPHA_FLOOR) & (al[1] >= ALPHA_FLOOR)      # the order matters only where both contribute
                    fragile[ya:yb, xa:xb] |= hit
                    fal[ya:yb, xa:xb] += np.where(hit, al[0] + al[1], 0.0)


# ---- image metrics (the reference's evaluation_utils formulas) in float64 -------------------------------------------------------
def window_1d(size=11, sigma=1.5):
    g = np.exp(-((np.arange(size) - size // 2) ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def _conv(img, w2):
    k = w2.shape[0]
    pad = k // 2
    p = np.pad(img, ((0, 0), (pad, pad), (pad, pad)))
    out = np.zeros_like(img)
    for dy in range(k):
        for dx in range(k):
            out += w2[dy, dx] * p[:, dy:dy + img.shape[1], dx:dx + img.shape[2]]
    return out


def metrics64(a, b):
    """-> (mse, psnr, ssim) of two (3,H,W) images, float64 throughout"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = window_1d()
    w2 = np.outer(g, g)
    mu1, mu2 = _conv(a, w2), _conv(b, w2)
    s1, s2, s12 = _conv(a * a, w2) - mu1 * mu1, _conv(b * b, w2) - mu2 * mu2, _conv(a * b, w2) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()
    mse = ((a - b) ** 2).mean()
    with np.errstate(divide="ignore"):
        psnr = 20.0 * np.log10(1.0 / np.sqrt(mse))
    return float(mse), float(psnr), float(ssim)


def image_pairs():
    """name -> (a, b), (3,H,W) float32 in [0, 1]: the pairs tests/golden/eval_metrics.npz holds the reference's metrics of"""
    rng = np.random.default_rng(2024)
    pairs = {}
    for tag, (h, w) in (("s", (48, 64)), ("l", (131, 203))):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([0.5 + 0.4 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)]).astype(np.float32)
        base = np.clip(base + rng.normal(0, 0.05, base.shape).astype(np.float32), 0, 1)
        pairs[f"identical_{tag}"] = (base, base.copy())
        pairs[f"noisy_{tag}"] = (base, np.clip(base + rng.normal(0, 0.1, base.shape), 0, 1).astype(np.float32))
        pairs[f"shifted_{tag}"] = (base, np.roll(base, (2, 3), (1, 2)))
        pairs[f"constant_{tag}"] = (np.full_like(base, 0.25), np.full_like(base, 0.75))
    return pairs


# ---- the test scenes, shared by tests/golden/make_golden_eval.py, tests/test_raster_cpu.py and tests/test_raster_gpu.py -------------
def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """float32 world -> camera matrix of a camera at ``eye`` looking at ``target`` (+z forward, +y down)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(np.asarray(up, np.float64), fwd)          # x = down x forward ... with y pointing down: x = y x z
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = -R @ eye
    return V.astype(np.float32)


def make_camera(eye, target, width, height, focal, up=(0.0, -1.0, 0.0)):
    return dict(viewmat=look_at(eye, target, up), fx=float(focal), fy=float(focal) * 1.05, cx=width / 2.0, cy=height / 2.0, width=width, height=height)


def _cov6(rng, n, lo, hi):
    s = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 3)))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    L = R * s[:, None, :]
    C = L @ L.transpose(0, 2, 1)
    return C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(np.float32)


def make_scene(n, seed, sh_degree, giants=0, tiny=0, spread=1.0):
    """``n`` splats in the box [-spread, spread]^3 (some therefore behind or beside the cameras placed near it), ``giants`` splats
    wide enough to cover every tile and ``tiny`` splats in a cluster whose radius sits at or under the 3-pixel clip.  Colours stay
    within [0, 1] for every direction (DC in [0.2, 0.8], small rest coefficients)."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-spread, spread, (n, 3))
    cov6 = _cov6(rng, n, 0.01, 0.08)
    if giants:
        xyz[:giants] = rng.uniform(-0.2, 0.2, (giants, 3))
        cov6[:giants] = _cov6(rng, giants, 1.5, 3.0)
    if tiny:
        xyz[giants:giants + tiny] = np.array([0.3, -0.2, 0.1]) + rng.normal(0, 0.05, (tiny, 3))
        cov6[giants:giants + tiny] = _cov6(rng, tiny, 0.004, 0.03)
    K = (sh_degree + 1) ** 2 - 1
    color = ((rng.uniform(0.2, 0.8, (n, 3)) - 0.5) / C0).astype(np.float32)
    sh = rng.normal(0, 0.02, (n, 3 * K)).astype(np.float32)
    opacity = rng.normal(0.5, 2.0, n).astype(np.float32)
    if giants:
        opacity[:giants] = -2.0                       # faint: the splats behind them still show
    return dict(xyz=xyz.astype(np.float32), cov6=cov6, opacity=opacity, color=color, sh=sh, sh_degree=sh_degree)


CAM_A = dict(eye=(0.3, -0.4, -3.2), target=(0.0, 0.0, 0.0))
CAM_B = dict(eye=(2.1, 0.6, -1.4), target=(0.1, -0.1, 0.2))          # close to the box: splats behind it and beyond the frame

# name -> (scene arguments, camera arguments, background, scale)
SCENES = {
    "deg0_black": (dict(n=1500, seed=11, sh_degree=0), dict(CAM_A, width=128, height=96, focal=110.0), (0.0, 0.0, 0.0), 1.0),
    "deg3_white_odd": (dict(n=2000, seed=12, sh_degree=3), dict(CAM_B, width=203, height=131, focal=150.0), (1.0, 1.0, 1.0), 1.0),
    "giants_tiny": (dict(n=1200, seed=13, sh_degree=3, giants=3, tiny=150), dict(CAM_A, width=256, height=192, focal=200.0), (0.1, 0.5, 0.9), 1.0),
    "scaled": (dict(n=1000, seed=14, sh_degree=1), dict(CAM_B, width=100, height=70, focal=90.0), (0.0, 0.0, 0.0), 1.7),
    "inside": (dict(n=3000, seed=15, sh_degree=2, spread=1.5), dict(eye=(0.2, 0.1, -0.3), target=(0.0, 0.3, 1.0), width=160, height=120, focal=100.0),
               (0.3, 0.3, 0.3), 1.0),
}
# a scene with no fragile pixel (asserted in tests/test_raster_cpu.py): its counts must equal the kernel's exactly
EXACT_SCENE = "exact"
SCENES[EXACT_SCENE] = (dict(n=60, seed=21, sh_degree=1), dict(CAM_A, width=96, height=80, focal=80.0), (0.2, 0.2, 0.2), 1.0)


def build(name):
    """-> (scene with the covariances already scaled, camera dict, background)"""
    sargs, cargs, bg, scale = SCENES[name]
    scene = make_scene(**sargs)
    scene["scale"] = scale
    return scene, make_camera(**cargs), bg


def scaled(scene):
    """the scene as the rasteriser sees it: cov6 * scale^2 in float32 (GaussianModel.get_full_covariance(scale))"""
    s = dict(scene)
    if scene.get("scale", 1.0) != 1.0:
        s["cov6"] = (np.asarray(scene["cov6"], np.float32) * np.float32(float(scene["scale"]) ** 2)).astype(np.float32)
    return s
