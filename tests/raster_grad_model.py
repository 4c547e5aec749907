"""NumPy statement of the rasteriser's backward pass (the header comment of ``gsr_raster_backward``): an ANALYTIC backward
of the forward ``raster_model`` states, the model ``k_raster_blend_bwd`` and ``k_raster_splat_bwd`` are held to.

``backward(scene, cam, G_C, G_A, background, dtype)``: float64 by default; with ``dtype=np.float32`` it follows the kernels' operation
order -- the forward walk, the backward walk with the recurrence ``T <- T / (1 - alpha)`` from ``T_end``, the tile tree (adjacent pairs
along a pixel row, rows in adjacent pairs inside a wave, the four waves in order), the per-splat sum over the tiles of its box in
row-major order, and the projection chain backwards.  ``raster_model.render`` does the same for the forward.  It returns the five
gradients, the nine per-splat sums ``g9`` (mean2d x y, conic A B C, opacity, r g b), ``abs9`` -- the per-splat sum of the ABSOLUTE values of
the terms of each of the nine sums -- and ``scale``: per output array, ``sum_k |d out / d sum_k| abs9_k`` (the chain is linear in the nine
sums), the magnitude against which an error of that output is read.

Every discrete decision is held at the value the forward took; ``switches(scene, cam)`` lists how far the three decisions that only
the backward pass looks at -- the 0.999 clamp per (splat, pixel), the colour clamp per (splat, channel), the frustum clamp of the
Jacobian per (splat, axis) -- sit from their switch.

``grad_edges`` is the scene built for this pass (see ``make_grad_edges``).
"""
from __future__ import annotations

import functools

import numpy as np

import raster_model as M

TILE = M.TILE
NAMES = ("mean_x", "mean_y", "conic_a", "conic_b", "conic_c", "opacity", "r", "g", "b")
OUTPUTS = ("xyz", "cov6", "raw_opacity", "dc", "sh_rest")
TINY = 1e-30


def tile_fold(v):
    """(..., 16 rows, 16 columns) -> (...): the fixed tree of k_raster_blend_bwd"""
    for _ in range(4):                                  # adjacent pairs along the pixel row (the four row_shr steps)
        v = v[..., 0::2] + v[..., 1::2]
    v = v[..., 0]
    v = v[..., 0::2] + v[..., 1::2]                     # rows 0 + 1, 2 + 3 of a wave (row_bcast15)
    v = v[..., 0::2] + v[..., 1::2]                     # the wave (row_bcast31)
    return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]


def _box_sum(terms, nty, ntx):
    """(9, h, w) terms over a splat's pixel box (clipped at the image) -> (9,): tile tree, then the tiles in row-major order, one after the other"""
    k, h, w = terms.shape
    full = np.zeros((k, nty * TILE, ntx * TILE), terms.dtype)
    full[:, :h, :w] = terms
    tiles = tile_fold(full.reshape(k, nty, TILE, ntx, TILE).transpose(0, 1, 3, 2, 4)).reshape(k, nty * ntx)
    return np.cumsum(tiles, axis=1, dtype=terms.dtype)[:, -1]


def pixel_pass(scene, cam, G_C, G_A, background=(0.0, 0.0, 0.0), dtype=np.float64, radius_clip=3.0):
    """the two walks over the pixels -> dict(g9 (n,9) in dtype, abs9 (n,9) float64, P, order, T_end, counted: splat -> (slice, mask of the
    pixels that counted it, mask of those where the 0.999 clamp was active))"""
    f = np.dtype(dtype).type
    P = M.project(scene, cam, dtype, radius_clip)
    W, H = P["W"], P["H"]
    n = len(P["ok"])
    vis = np.nonzero(P["ok"])[0]
    order = vis[np.lexsort((vis, P["z"][vis]))]
    T = np.ones((H, W), dtype)
    done = np.zeros((H, W), bool)
    steps = []
    for i in order:                                     # the forward walk, as raster_model.render
        xa, xb, ya, yb = P["x0"][i] * TILE, min(P["x1"][i] * TILE, W), P["y0"][i] * TILE, min(P["y1"][i] * TILE, H)
        xs, ys = np.arange(xa, xb), np.arange(ya, yb)
        sigma, alpha, _ = M._alpha(P, i, xs, ys, f)
        sl = (slice(ya, yb), slice(xa, xb))
        keep = ~done[sl] & ~(sigma < 0) & ~(alpha < f(1.0) / f(255.0))
        Tn = T[sl] * (f(1) - alpha)
        stop = keep & (Tn <= f(1e-4))
        upd = keep & ~stop
        T[sl] = np.where(upd, Tn, T[sl])
        done[sl] |= stop
        steps.append((i, sl, xs, ys, sigma, alpha, upd))
    T_end = T.copy()
    gC = np.asarray(G_C, np.float32).astype(dtype) if G_C is not None else np.zeros((H, W, 3), dtype)
    gA = np.asarray(G_A, np.float32).astype(dtype) if G_A is not None else np.zeros((H, W), dtype)
    bg = np.asarray(background, np.float32).astype(dtype)
    tga = T_end * gA
    acc = T_end * ((bg[0] * gC[..., 0] + bg[1] * gC[..., 1]) + bg[2] * gC[..., 2])
    g9 = np.zeros((n, 9), dtype)
    abs9 = np.zeros((n, 9), np.float64)
    counted = {}
    zero = f(0)
    for i, sl, xs, ys, sigma, alpha, upd in reversed(steps):
        dx = (P["mx"][i] - (xs.astype(dtype) + f(0.5)))[None, :]
        dy = (P["my"][i] - (ys.astype(dtype) + f(0.5)))[:, None]
        A, B, C = P["conic"][i]
        with np.errstate(over="ignore"):
            e = np.exp(-sigma)
        araw = P["op"][i] * e
        om = f(1) - alpha
        Tk = np.where(upd, T[sl] / om, T[sl])
        T[sl] = Tk
        w = alpha * Tk
        g = gC[sl]
        c = P["rgb"][i]
        cg = (c[0] * g[..., 0] + c[1] * g[..., 1]) + c[2] * g[..., 2]
        dalpha = Tk * cg - (acc[sl] - tga[sl]) / om
        acc[sl] = np.where(upd, acc[sl] + w * cg, acc[sl])
        clamped = araw > f(0.999)
        free = upd & ~clamped
        gs = -(alpha * dalpha)
        terms = np.stack([np.where(free, gs * (A * dx + B * dy), zero), np.where(free, gs * (C * dy + B * dx), zero),
                          np.where(free, gs * (f(0.5) * (dx * dx)), zero), np.where(free, gs * (dx * dy), zero),
                          np.where(free, gs * (f(0.5) * (dy * dy)), zero), np.where(free, e * dalpha, zero),
                          np.where(upd, w * g[..., 0], zero), np.where(upd, w * g[..., 1], zero), np.where(upd, w * g[..., 2], zero)])
        nty, ntx = int(P["y1"][i] - P["y0"][i]), int(P["x1"][i] - P["x0"][i])
        g9[i] = _box_sum(terms, nty, ntx)
        abs9[i] = np.abs(terms.astype(np.float64)).sum(axis=(1, 2))
        counted[int(i)] = (sl, upd, upd & clamped)
    return dict(g9=g9, abs9=abs9, P=P, order=order, T_end=T_end, counted=counted, stopped=done)


def _forward_chain_values(scene, cam, dtype):
    """the values of k_raster_preprocess the chain needs, in ``dtype`` with the kernel's expressions"""
    f = np.dtype(dtype).type
    V = np.asarray(cam["viewmat"], np.float32).reshape(4, 4)
    R, t = V[:3, :3].astype(dtype), V[:3, 3].astype(dtype)
    campos = (-(V[:3, :3].astype(np.float64).T @ V[:3, 3].astype(np.float64))).astype(np.float32).astype(dtype)
    W, H = int(cam["width"]), int(cam["height"])
    fx, fy, cx, cy = (f(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    p = np.asarray(scene["xyz"], np.float32).astype(dtype)
    c6 = np.asarray(scene["cov6"], np.float32).astype(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    pc = [((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)]
    S = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
    Mx = [[(R[r, 0] * S[0][q] + R[r, 1] * S[1][q]) + R[r, 2] * S[2][q] for q in range(3)] for r in range(3)]
    Sc = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for q in range(r, 3):
            Sc[r][q] = Sc[q][r] = (Mx[r][0] * R[q, 0] + Mx[r][1] * R[q, 1]) + Mx[r][2] * R[q, 2]
    tan_x, tan_y = f(0.5) * f(W) / fx, f(0.5) * f(H) / fy
    lim_xp, lim_xn = (f(W) - cx) / fx + f(0.3) * tan_x, cx / fx + f(0.3) * tan_x
    lim_yp, lim_yn = (f(H) - cy) / fy + f(0.3) * tan_y, cy / fy + f(0.3) * tan_y
    return dict(f=f, R=R, campos=campos, fx=fx, fy=fy, p=p, pc=pc, Sc=Sc, lims=(lim_xp, lim_xn, lim_yp, lim_yn))


def _basis_and_derivatives(degree, d):
    """-> list of (b_k, db_k/dx, db_k/dy, db_k/dz) along the unit vectors d (n,3), the basis as raster_model.sh_basis"""
    f = d.dtype.type
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    o = np.zeros_like(x)
    C1, C2, C3 = f(M.C1), [f(v) for v in M.C2], [f(v) for v in M.C3]
    out = []
    if degree > 0:
        out += [(-C1 * y, o, o - C1, o), (C1 * z, o, o, o + C1), (-C1 * x, o - C1, o, o)]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        out += [(C2[0] * xy, C2[0] * y, C2[0] * x, o), (C2[1] * yz, o, C2[1] * z, C2[1] * y),
                (C2[2] * (f(2) * zz - xx - yy), C2[2] * (f(-2) * x), C2[2] * (f(-2) * y), C2[2] * (f(4) * z)),
                (C2[3] * xz, C2[3] * z, o, C2[3] * x), (C2[4] * (xx - yy), C2[4] * (f(2) * x), C2[4] * (f(-2) * y), o)]
    if degree > 2:
        out += [(C3[0] * y * (f(3) * xx - yy), C3[0] * (f(6) * xy), C3[0] * (f(3) * xx - f(3) * yy), o),
                (C3[1] * xy * z, C3[1] * yz, C3[1] * xz, C3[1] * xy),
                (C3[2] * y * (f(4) * zz - xx - yy), C3[2] * (f(-2) * xy), C3[2] * (f(4) * zz - xx - f(3) * yy), C3[2] * (f(8) * yz)),
                (C3[3] * z * (f(2) * zz - f(3) * xx - f(3) * yy), C3[3] * (f(-6) * xz), C3[3] * (f(-6) * yz), C3[3] * (f(6) * zz - f(3) * xx - f(3) * yy)),
                (C3[4] * x * (f(4) * zz - xx - yy), C3[4] * (f(4) * zz - f(3) * xx - yy), C3[4] * (f(-2) * xy), C3[4] * (f(8) * xz)),
                (C3[5] * z * (xx - yy), C3[5] * (f(2) * xz), C3[5] * (f(-2) * yz), C3[5] * (xx - yy)),
                (C3[6] * x * (xx - f(3) * yy), C3[6] * (f(3) * xx - f(3) * yy), C3[6] * (f(-6) * xy), o)]
    return out


def chain(scene, cam, P, g9, dtype=np.float64):
    """the projection backwards, k_raster_splat_bwd's expressions for all splats at once: (n,9) sums -> dict of the five gradients in
    ``dtype`` (zeros for culled splats).  Linear in g9."""
    v = _forward_chain_values(scene, cam, dtype)
    f, R, fx, fy, pc, Sc = v["f"], v["R"], v["fx"], v["fy"], v["pc"], v["Sc"]
    lim_xp, lim_xn, lim_yp, lim_yn = v["lims"]
    n = v["p"].shape[0]
    ok = P["ok"]
    g = [np.where(ok, g9[:, k].astype(dtype), f(0)) for k in range(9)]
    two, half = f(2), f(0.5)
    with np.errstate(all="ignore"):
        px, py, pz = pc
        rz = f(1) / pz
        ux, uy = px * rz, py * rz
        tx = pz * np.minimum(lim_xp, np.maximum(-lim_xn, ux))
        ty = pz * np.minimum(lim_yp, np.maximum(-lim_yn, uy))
        clx, cly = (ux > lim_xp) | (ux < -lim_xn), (uy > lim_yp) | (uy < -lim_yn)
        limx, limy = np.where(ux > lim_xp, lim_xp, -lim_xn), np.where(uy > lim_yp, lim_yp, -lim_yn)
        rz2 = rz * rz
        j00, j02, j11, j12 = fx * rz, -(fx * tx) * rz2, fy * rz, -(fy * ty) * rz2
        v00, v01, v02 = Sc[0][0] * j00 + Sc[0][2] * j02, Sc[1][0] * j00 + Sc[1][2] * j02, Sc[2][0] * j00 + Sc[2][2] * j02
        v11, v12 = Sc[1][1] * j11 + Sc[1][2] * j12, Sc[2][1] * j11 + Sc[2][2] * j12
        a = (j00 * v00 + j02 * v02) + f(M.EPS2D)
        b = j11 * v01 + j12 * v02
        c = (j11 * v11 + j12 * v12) + f(M.EPS2D)
        det = a * c - b * b
        di = f(1) / det
        di2 = di * di
        ga = di2 * (((b * c) * g[3] - (c * c) * g[2]) - (b * b) * g[4])
        gc = di2 * (((a * b) * g[3] - (b * b) * g[2]) - (a * a) * g[4])
        gb = di2 * (((two * (b * c)) * g[2] - (a * c + b * b) * g[3]) + (two * (a * b)) * g[4])
        s00, s01, s02 = ga * (j00 * j00), gb * (j00 * j11), ga * (two * (j00 * j02)) + gb * (j00 * j12)
        s11, s12 = gc * (j11 * j11), gb * (j02 * j11) + gc * (two * (j11 * j12))
        s22 = (ga * (j02 * j02) + gb * (j02 * j12)) + gc * (j12 * j12)
        G = [[s00, half * s01, half * s02], [half * s01, s11, half * s12], [half * s02, half * s12, s22]]
        N = [[(R[0, r] * G[0][q] + R[1, r] * G[1][q]) + R[2, r] * G[2][q] for q in range(3)] for r in range(3)]
        Gw = [[(N[r][0] * R[0, q] + N[r][1] * R[1, q]) + N[r][2] * R[2, q] for q in range(3)] for r in range(3)]
        g_cov6 = np.stack([Gw[0][0], two * Gw[0][1], two * Gw[0][2], Gw[1][1], two * Gw[1][2], Gw[2][2]], 1)
        op = P["op"]
        g_raw = g[5] * (op * (f(1) - op))
        rgb = P["rgb"]
        gv = [np.where(rgb[:, ch] > 0, g[6 + ch], f(0)) for ch in range(3)]
        g_dc = np.stack([f(M.C0) * gv[ch] for ch in range(3)], 1)
        d = v["p"] - v["campos"]
        il = f(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d * il[:, None]
        deg = int(scene["sh_degree"])
        rest = np.asarray(scene["sh"], np.float32).astype(dtype).reshape(n, -1, 3)
        K = rest.shape[1]
        g_rest = np.zeros((n, K, 3), dtype)
        gd = [np.zeros(n, dtype) for _ in range(3)]
        for k, (bk, ddx, ddy, ddz) in enumerate(_basis_and_derivatives(deg, d)):
            gbk = (rest[:, k, 0] * gv[0] + rest[:, k, 1] * gv[1]) + rest[:, k, 2] * gv[2]
            gd = [gd[0] + gbk * ddx, gd[1] + gbk * ddy, gd[2] + gbk * ddz]
            for ch in range(3):
                g_rest[:, k, ch] = bk * gv[ch]
        u = j11 * Sc[0][1] + j12 * Sc[0][2]
        gj00, gj02 = two * (ga * v00) + gb * u, two * (ga * v02) + gb * v12
        gj11, gj12 = gb * v01 + two * (gc * v11), gb * v02 + two * (gc * v12)
        rz3 = rz2 * rz
        gtx, gty = -(fx * rz2) * gj02, -(fy * rz2) * gj12
        gpx = g[0] * (fx * rz) + np.where(clx, f(0), gtx)
        gpy = g[1] * (fy * rz) + np.where(cly, f(0), gty)
        gpz = -(fx * rz2) * gj00 - (fy * rz2) * gj11
        gpz = gpz + ((two * (fx * tx)) * rz3) * gj02
        gpz = gpz + ((two * (fy * ty)) * rz3) * gj12
        gpz = gpz - (g[0] * (fx * px)) * rz2
        gpz = gpz - (g[1] * (fy * py)) * rz2
        gpz = gpz + np.where(clx, limx * gtx, f(0))
        gpz = gpz + np.where(cly, limy * gty, f(0))
        dg = (d[:, 0] * gd[0] + d[:, 1] * gd[1]) + d[:, 2] * gd[2]
        wv = [il * (gd[q] - d[:, q] * dg) for q in range(3)]
        g_xyz = np.stack([((R[0, q] * gpx + R[1, q] * gpy) + R[2, q] * gpz) + wv[q] for q in range(3)], 1)
    z1 = lambda arr: np.where(ok.reshape((n,) + (1,) * (arr.ndim - 1)), arr, f(0)).astype(dtype)
    return dict(xyz=z1(g_xyz), cov6=z1(g_cov6), raw_opacity=z1(g_raw), dc=z1(g_dc), sh_rest=z1(g_rest.reshape(n, 3 * K)))


def backward(scene, cam, G_C=None, G_A=None, background=(0.0, 0.0, 0.0), dtype=np.float64, radius_clip=3.0):
    """-> dict(xyz (n,3), cov6 (n,6), raw_opacity (n,), dc (n,3), sh_rest (n,3K) in dtype; g9, abs9; scale: output name -> array of its
    shape (float64 mode only); ok, P, counted)"""
    pp = pixel_pass(scene, cam, G_C, G_A, background, dtype, radius_clip)
    out = chain(scene, cam, pp["P"], pp["g9"], dtype)
    out.update(g9=pp["g9"], abs9=pp["abs9"], P=pp["P"], ok=pp["P"]["ok"], counted=pp["counted"], T_end=pp["T_end"], stopped=pp["stopped"])
    if np.dtype(dtype) == np.float64:
        scale = {k: np.zeros_like(out[k]) for k in OUTPUTS}
        n = len(pp["P"]["ok"])
        for k in range(9):
            unit = np.zeros((n, 9))
            unit[:, k] = 1.0
            jac = chain(scene, cam, pp["P"], unit, np.float64)
            for name in OUTPUTS:
                scale[name] += np.abs(jac[name]) * pp["abs9"][:, k].reshape((n,) + (1,) * (jac[name].ndim - 1))
        out["scale"] = scale
    return out


def switches(scene, cam, radius_clip=3.0):
    """How far the backward pass's own decisions sit from their switch, relative, in float64: dict(opacity_clamp: the least
    |op e / 0.999 - 1| over the (splat, pixel) pairs that count, colour: the least |v + 0.5| / (|C0 dc| + sum |b_k rest_k| + 0.5) over the
    visible (splat, channel) pairs, jacobian: the least |u / lim - 1| over the visible (splat, axis, side)), and the counts of active
    clamps of each kind among the visible splats."""
    P = M.project(scene, cam, np.float64, radius_clip)
    pp = pixel_pass(scene, cam, None, np.zeros((P["H"], P["W"])), (0.0, 0.0, 0.0), np.float64, radius_clip)
    ok = P["ok"]
    n = len(ok)
    m_op, n_op = np.inf, 0
    for i, (sl, upd, clamped) in pp["counted"].items():
        ya, yb, xa, xb = sl[0].start, sl[0].stop, sl[1].start, sl[1].stop
        sigma = M._alpha(P, i, np.arange(xa, xb), np.arange(ya, yb), np.float64)[0]
        with np.errstate(over="ignore"):
            araw = P["op"][i] * np.exp(-sigma)
        if upd.any():
            m_op = min(m_op, float(np.abs(araw[upd] / 0.999 - 1.0).min()))
        n_op += int(clamped.any())
    v = _forward_chain_values(scene, cam, np.float64)
    d = v["p"] - v["campos"]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    basis = M.sh_basis(int(scene["sh_degree"]), d)
    dc = np.asarray(scene["color"], np.float64)
    rest = np.asarray(scene["sh"], np.float64).reshape(n, -1, 3)
    val = M.C0 * dc + np.einsum("nk,nkc->nc", basis, rest[:, :basis.shape[1]]) + 0.5
    mag = np.abs(M.C0 * dc) + np.einsum("nk,nkc->nc", np.abs(basis), np.abs(rest[:, :basis.shape[1]])) + 0.5
    m_col = float((np.abs(val) / mag)[ok].min()) if ok.any() else np.inf
    lim_xp, lim_xn, lim_yp, lim_yn = v["lims"]
    with np.errstate(all="ignore"):
        ux, uy = v["pc"][0] / v["pc"][2], v["pc"][1] / v["pc"][2]
    rel = np.stack([np.abs(ux / lim_xp - 1), np.abs(ux / -lim_xn - 1), np.abs(uy / lim_yp - 1), np.abs(uy / -lim_yn - 1)], 1)
    m_jac = float(rel[ok].min()) if ok.any() else np.inf
    jac_active = ok & ((ux > lim_xp) | (ux < -lim_xn) | (uy > lim_yp) | (uy < -lim_yn))
    return dict(opacity_clamp=m_op, colour=m_col, jacobian=m_jac, opacity_clamped_splats=n_op, colour_clamped=int(((val <= 0) & ok[:, None]).sum()),
                jacobian_clamped_splats=int(jac_active.sum()), jac_active=jac_active, colour_off=(val <= 0) & ok[:, None])


# ---- the scene of the backward pass's edge cases ---------------------------------------------------------------------------------
GRAD_EDGES = "grad_edges"
EDGE_CAM = dict(eye=(0.0, 0.0, -3.0), target=(0.0, 0.0, 0.0), width=41, height=27, focal=40.0)
EDGE_BG = (0.3, 0.6, 0.1)
# rows of the scene (make_grad_edges): the splats the tests name
ROW_CLAMPED_OPACITY, ROW_CLAMPED_COLOUR, ROW_CLAMPED_JACOBIAN, ROW_EVERY_TILE, ROW_EQUAL_DEPTH = 0, 1, 2, 3, (4, 5)
ROW_BEHIND = (6, 7, 8)
ROW_STACK = 9                          # 300 faint splats from here, all inside one tile
STACK = 300
ROW_STOP = ROW_STACK + STACK           # 14 nearly opaque splats on one spot: the 1e-4 stop
STOPPERS = 14
ROW_FILL = ROW_STOP + STOPPERS         # 30 ordinary splats
FILL = 30


def _iso(s):
    return [s * s, 0.0, 0.0, s * s, 0.0, s * s]


def coarse(scene, bits=11):
    """the scene with every array rounded to ``bits`` significant bits: a step of 2^-20 relative to a value's own power of two then
    adds to it exactly in float32 (the forward model narrows its inputs to float32 first), which finite differences need"""
    def q(a):
        a = np.asarray(a, np.float64)
        e = np.floor(np.log2(np.where(a == 0, 1.0, np.abs(a))))
        step = 2.0 ** (e - (bits - 1))
        return (np.round(a / step) * step).astype(np.float32)
    out = dict(scene)
    for k in ("xyz", "cov6", "opacity", "color", "sh"):
        out[k] = q(scene[k])
    return out


def make_grad_edges():
    """41 x 27 pixels (3 x 2 tiles, partial at both edges), SH degree 1, the camera at (0, 0, -3) looking along +z (camera x, y = -world
    x, y), every value rounded to 11 significant bits (``coarse``).  Row by row:
    0: raw opacity 9, wide (sigma about 8 px), its mean within 0.05 px of a pixel centre: alpha is clamped at 0.999 on that pixel;
    1: a colour whose red channel is clamped at 0 (DC far below -0.5 / C0);
    2: a large faint splat centred far beside the frame, beyond the widened frustum: the x/z clamp of the Jacobian is active;
    3: one faint splat wide enough to cover every tile;
    4, 5: two small splats at exactly the same float32 depth in one tile, overlapping on a few pixels (fragile: the order decides);
    6 .. 8: behind the camera (culled);
    9 .. 308: 300 faint small splats stacked inside the tile (1, 0), at increasing depth: two LDS batches in that tile;
    309 .. 322: 14 nearly opaque splats on one spot behind each other: the stack reaches the 1e-4 stop;
    323 .. 352: ordinary splats."""
    rng = np.random.default_rng(2600)
    n = ROW_FILL + FILL
    f, W, H = EDGE_CAM["focal"], EDGE_CAM["width"], EDGE_CAM["height"]

    def place(u, v, z):
        """the world point at height z that projects to pixel coordinates (u, v)"""
        u, v, z = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(z, np.float64)
        return np.stack(np.broadcast_arrays(-(u - W / 2.0) * (z + 3.0) / f, -(v - H / 2.0) * (z + 3.0) / (1.05 * f), z), -1)
    xyz = np.zeros((n, 3))
    cov6 = np.zeros((n, 6))
    opacity = np.zeros(n)
    color = ((rng.uniform(0.25, 0.75, (n, 3)) - 0.5) / M.C0)
    sh = rng.normal(0, 0.02, (n, 9))
    xyz[0], cov6[0], opacity[0] = place(10.5, 8.5, 0.25), _iso(0.7), 9.0
    xyz[1], cov6[1], opacity[1] = place(30.2, 20.3, 0.125), _iso(0.3), 0.5
    color[1, 0] = (-0.4 - 0.5) / M.C0
    xyz[2], cov6[2], opacity[2] = (-5.25, 0.1875, 0.625), _iso(1.3), -1.0
    xyz[3], cov6[3], opacity[3] = (0.09375, -0.046875, 1.5), _iso(2.5), -2.5
    xyz[4], cov6[4], opacity[4] = place(33.3, 20.7, 0.5), _iso(0.09), 0.3          # small: where both count, the order is fragile
    xyz[5], cov6[5], opacity[5] = place(39.4, 21.6, 0.5), _iso(0.095), 0.8
    for k, r in enumerate(ROW_BEHIND):
        xyz[r], cov6[r], opacity[r] = (0.2 * k, 0.1, -4.0 - k), _iso(0.3), 1.0
    s = slice(ROW_STACK, ROW_STACK + STACK)           # tile (1, 0): pixels 16 .. 31 x 0 .. 15; the 3-sigma radius stays inside it
    xyz[s] = place(rng.uniform(21.5, 26.5, STACK), rng.uniform(5.5, 10.5, STACK), np.linspace(-0.5, 0.4, STACK))
    cov6[s] = np.float64(_iso(0.075))
    opacity[s] = rng.uniform(-4.2, -3.6, STACK)
    s = slice(ROW_STOP, ROW_STOP + STOPPERS)
    xyz[s] = place(8.4, 19.6, np.linspace(0.8, 1.4, STOPPERS))
    cov6[s] = np.float64(_iso(0.35))
    opacity[s] = 2.2
    s = slice(ROW_FILL, n)
    xyz[s] = rng.uniform((-1.4, -0.9, -0.6), (1.4, 0.9, 1.2), (FILL, 3))
    cov6[s] = M._cov6(rng, FILL, 0.05, 0.3)
    opacity[s] = rng.normal(0.0, 1.5, FILL)
    return coarse(dict(xyz=xyz, cov6=cov6, opacity=opacity, color=color, sh=sh, sh_degree=1, scale=1.0))


GPU_SCENES = (M.EXACT_SCENE, "deg3_white_odd", "giants_tiny", "scaled", GRAD_EDGES)


def build(name):
    """-> (scene as the rasteriser sees it, camera dict, background), of ``raster_model.SCENES`` or ``grad_edges``"""
    if name == GRAD_EDGES:
        return make_grad_edges(), M.make_camera(**EDGE_CAM), EDGE_BG
    scene, cam, bg = M.build(name)
    return M.scaled(scene), cam, bg


def upstream(name, H, W):
    """the fixed random G_C (H,W,3) and G_A (H,W) of a scene, float32 values"""
    rng = np.random.default_rng(abs(hash_name(name)))
    return rng.normal(0, 1, (H, W, 3)).astype(np.float32), rng.normal(0, 1, (H, W)).astype(np.float32)


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) + 977


@functools.lru_cache(maxsize=None)
def scene_models(name):
    """Everything the tests need of a scene, computed once and left unchanged: scene, cam, bg, the float64 forward (fragile mask, counts),
    G_C and G_A zeroed on the fragile pixels, and the float64 backward of both, of G_C alone and of G_A alone."""
    scene, cam, bg = build(name)
    ref = M.render(scene, cam, bg)
    H, W = ref["fragile"].shape
    G_C, G_A = upstream(name, H, W)
    G_C[ref["fragile"]] = 0.0
    G_A[ref["fragile"]] = 0.0
    both = backward(scene, cam, G_C, G_A, bg)
    for a in (G_C, G_A, ref["fragile"], ref["image"]):
        a.setflags(write=False)
    for k in OUTPUTS:
        both[k].setflags(write=False)
        both["scale"][k].setflags(write=False)
    return dict(scene=scene, cam=cam, bg=bg, ref=ref, G_C=G_C, G_A=G_A, both=both)


def float32_cost(name):
    """what float32 costs the model itself: per output array, max |g32 - g64| / (scale + TINY) over all splats"""
    m = scene_models(name)
    g32 = backward(m["scene"], m["cam"], m["G_C"], m["G_A"], m["bg"], np.float32)
    g64 = m["both"]
    return {k: float((np.abs(g32[k].astype(np.float64) - g64[k]) / (g64["scale"][k] + TINY)).max()) for k in OUTPUTS}
