"""NumPy float64 restatement of the photometric refinement: the sums ``gsr_photo_accumulate`` is held to, the damped
Gauss-Newton loop of ``photo.PhotometricRefiner``, and the scenes the tests use.  The hybrid term of Open3D's RGB-D odometry (Park,
Zhou, Koltun 2017), restated for rendered maps and a world-frame increment.  Parity with Open3D is unpinned.

One camera: ``V = [R_c | t_c]`` world -> camera, ``fx fy cx cy``, ``W x H``.  TARGET maps ``I_t (H,W,3)``, ``D_t``, ``A_t (H,W)``: the
render of the target model; SOURCE maps ``I_s, D_s, A_s``: the render of the source model through ``V T`` (``T`` the current rigid
estimate).  All float32.  Every quantity below is float64 computed from them, every sum of three products is taken left to right,
``(a + b) + c``, no fused multiply-add: ``accumulate`` and the kernel compute every per-pixel term with the same operations in the
same order, so that they differ by the order of the SUMMATION alone.

A pixel ``(ix, iy)`` COUNTS when (each comparison in float64, on the float32 values widened exactly; a NaN fails all of them)
  ``A_s >= tau``,
  all nine target pixels of its 3 x 3 neighbourhood are inside the image and have ``A_t >= tau`` (border pixels never count),
  ``|D_t - D_s| <= max_depth_diff`` (the difference of the two widened values, one float64 subtraction).
``D_s > 0`` on a counted pixel is the renderer's promise (its near plane is 0.01), not a gate.

Per counted pixel, ``Y = (0.299 r + 0.587 g) + 0.114 b``, ``u = ix + 0.5``, ``v = iy + 0.5``, ``z = D_s``:
  ``p = (z xn, z yn, z)`` with ``xn = (u - cx) / fx``, ``yn = (v - cy) / fy``;  ``q = p - t_c``;  ``p_w = R_c' q``;
  ``M = R_c [-[p_w]x | I]`` (3 x 6: ``xi = (omega, v)``, rotation first, the left perturbation ``T <- [exp(omega) | v] T``);
  Sobel gradients of the target maps over 8: ``g = ((t(-1) + 2 t(0)) + t(+1)) / 8`` with ``t(k)`` the difference of the two taps of row
  (column) ``k``;
  ``a = ((gYx fx) / z, (gYy fy) / z, -(a0 X + a1 Y) / z)`` and ``d = ((gDx fx) / z, (gDy fy) / z, -(d0 X + d1 Y) / z - 1)``;
  ``J_I = sI (a M)``, ``J_D = sD (d M)``, ``r_I = sI (Y_t - Y_s)``, ``r_D = sD (D_t - z)``, ``sI = sqrt(1 - lambda)``, ``sD = sqrt(lambda)``.
The 30 sums, ``NSUMS``: [0..20] the upper triangle of ``sum (J_I' J_I + J_D' J_D)`` row by row, [21..26] ``sum (J_I' r_I + J_D' r_D)``,
[27] ``sum r_I^2``, [28] ``sum r_D^2``, [29] the count.  A pixel's TERM of a sum is what it adds (e.g. ``J_I[k] J_I[l] + J_D[k] J_D[l]``).
"""
from __future__ import annotations

import numpy as np

NSUMS = 30
LAMBDA, TAU = 0.968, 0.5
TRIU = [(r, c) for r in range(6) for c in range(r, 6)]


def intensity(img):
    img = np.asarray(img, np.float32).astype(np.float64)
    return (0.299 * img[..., 0] + 0.587 * img[..., 1]) + 0.114 * img[..., 2]


def _sobel(F):
    """(gx, gy) on the interior (H-2, W-2) of a float64 map"""
    c = lambda dy, dx: F[1 + dy:F.shape[0] - 1 + dy, 1 + dx:F.shape[1] - 1 + dx]
    gx = (((c(-1, 1) - c(-1, -1)) + 2.0 * (c(0, 1) - c(0, -1))) + (c(1, 1) - c(1, -1))) * 0.125
    gy = (((c(1, -1) - c(-1, -1)) + 2.0 * (c(1, 0) - c(-1, 0))) + (c(1, 1) - c(-1, 1))) * 0.125
    return gx, gy


def counted(src, tgt, tau, max_depth_diff):
    """(H, W) bool: the pixels that count"""
    As, At = (np.asarray(m["alpha"], np.float32).astype(np.float64) for m in (src, tgt))
    Ds, Dt = (np.asarray(m["depth"], np.float32).astype(np.float64) for m in (src, tgt))
    H, W = As.shape
    ok = np.zeros((H, W), bool)
    if H < 3 or W < 3:
        return ok
    with np.errstate(invalid="ignore"):
        t = At >= tau
        nine = np.ones((H - 2, W - 2), bool)
        for dy in range(3):
            for dx in range(3):
                nine &= t[dy:H - 2 + dy, dx:W - 2 + dx]
        ok[1:-1, 1:-1] = nine
        ok &= (As >= tau) & (np.abs(Dt - Ds) <= max_depth_diff)
    return ok


def gate_margins(src, tgt, tau, max_depth_diff):
    """the smallest distances of any pixel's values from the gates: (|A_s - tau|, |A_t - tau|, ||D_t - D_s| - max_depth_diff|)"""
    As, At = (np.asarray(m["alpha"], np.float32).astype(np.float64) for m in (src, tgt))
    Ds, Dt = (np.asarray(m["depth"], np.float32).astype(np.float64) for m in (src, tgt))
    return float(np.abs(As - tau).min()), float(np.abs(At - tau).min()), float(np.abs(np.abs(Dt - Ds) - max_depth_diff).min())


def accumulate(src, tgt, cam, lam=LAMBDA, tau=TAU, max_depth_diff=None):
    """-> (sums (30,), abs_sums (30,)): the sums of one camera and, beside each, the sum of the absolute values of its terms.
    ``src`` / ``tgt``: dict(image (H,W,3), depth (H,W), alpha (H,W)); ``cam``: dict(viewmat (4,4), fx, fy, cx, cy, width, height)."""
    V = np.asarray(cam["viewmat"], np.float64).reshape(4, 4)
    R, t = V[:3, :3], V[:3, 3]
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    sI, sD = np.sqrt(1.0 - lam), np.sqrt(lam)
    ok = counted(src, tgt, tau, max_depth_diff)
    sums, asum = np.zeros(NSUMS), np.zeros(NSUMS)
    if not ok.any():
        return sums, asum
    Ds, Dt = (np.asarray(m["depth"], np.float32).astype(np.float64) for m in (src, tgt))
    Ys, Yt = intensity(src["image"]), intensity(tgt["image"])
    H, W = Ds.shape
    gYx, gYy = (np.pad(g, 1) for g in _sobel(Yt))
    gDx, gDy = (np.pad(g, 1) for g in _sobel(Dt))
    iy, ix = np.nonzero(ok)
    u, v = ix + 0.5, iy + 0.5
    z, dt = Ds[iy, ix], Dt[iy, ix]
    xn, yn = (u - cx) / fx, (v - cy) / fy
    X, Y = z * xn, z * yn
    q = [X - t[0], Y - t[1], z - t[2]]
    pw = [(R[0, i] * q[0] + R[1, i] * q[1]) + R[2, i] * q[2] for i in range(3)]
    M = [[R[r, 2] * pw[1] - R[r, 1] * pw[2], R[r, 0] * pw[2] - R[r, 2] * pw[0], R[r, 1] * pw[0] - R[r, 0] * pw[1],
          np.full_like(z, R[r, 0]), np.full_like(z, R[r, 1]), np.full_like(z, R[r, 2])] for r in range(3)]

    def row(gx, gy, minus):
        a0, a1 = (gx[iy, ix] * fx) / z, (gy[iy, ix] * fy) / z
        a2 = -((a0 * X + a1 * Y) / z) - minus
        return a0, a1, a2
    a, d = row(gYx, gYy, 0.0), row(gDx, gDy, 1.0)
    JI = [sI * ((a[0] * M[0][k] + a[1] * M[1][k]) + a[2] * M[2][k]) for k in range(6)]
    JD = [sD * ((d[0] * M[0][k] + d[1] * M[1][k]) + d[2] * M[2][k]) for k in range(6)]
    rI, rD = sI * (Yt[iy, ix] - Ys[iy, ix]), sD * (dt - z)
    terms = [JI[r] * JI[c] + JD[r] * JD[c] for r, c in TRIU] + [JI[k] * rI + JD[k] * rD for k in range(6)] + [rI * rI, rD * rD, np.ones_like(z)]
    for k, term in enumerate(terms):
        sums[k], asum[k] = term.sum(), np.abs(term).sum()
    return sums, asum


def unpack(sums):
    """-> (H (6,6), b (6,), e_I, e_D, n) of the 30 sums"""
    Hm = np.zeros((6, 6))
    for k, (r, c) in enumerate(TRIU):
        Hm[r, c] = Hm[c, r] = sums[k]
    return Hm, np.array(sums[21:27], np.float64), float(sums[27]), float(sums[28]), float(sums[29])


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
RCOND = 1e-8


def solve_step(Hm, b, mu):
    """``-(H + mu I)^+ b``: eigenvalues below ``RCOND`` of the largest count as zero, so a direction the data do not constrain is left alone"""
    w, Q = np.linalg.eigh(Hm + mu * np.eye(6))
    keep = w > RCOND * max(w.max(), 0.0)
    inv = np.where(keep, 1.0 / np.where(keep, w, 1.0), 0.0)
    return -(Q @ (inv * (Q.T @ b)))


def se3_exp(xi):
    """4 x 4 of ``[exp(omega) | v]`` (the translation is v itself), xi = (omega, v)"""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        Rm = np.eye(3) + K
    else:
        Rm = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, v
    return T


def refine(render_source, targets, cams, T0, lam=LAMBDA, tau=TAU, max_depth_diff=None, max_iteration=30, min_increment=1e-9, mu0=0.0):
    """One pyramid level of the loop.  ``render_source(cam, T)`` -> the source maps through ``viewmat T``; ``targets[i]``: the target maps
    of ``cams[i]``.  -> dict(T, energies (of the start and of every accepted step), n, iterations, H (at the last accepted point))."""
    def evaluate(T):
        tot = np.zeros(NSUMS)
        for cam, tg in zip(cams, targets):
            tot += accumulate(render_source(cam, T), tg, cam, lam, tau, max_depth_diff)[0]
        Hm, b, eI, eD, n = unpack(tot)
        return Hm, b, ((eI + eD) / n if n else np.inf), n
    T = np.array(T0, np.float64)
    Hm, b, E, n = evaluate(T)
    energies, mu, it = [E], mu0, 0
    while it < max_iteration and n > 0:
        it += 1
        delta = solve_step(Hm, b, mu)
        Tn = se3_exp(delta) @ T
        Hn, bn, En, nn = evaluate(Tn)
        if nn > 0 and En <= E:
            T, Hm, b, E, n, mu = Tn, Hn, bn, En, nn, mu / 10.0
            energies.append(E)
            if np.linalg.norm(delta) < min_increment:
                break
        else:
            if np.linalg.norm(delta) < min_increment:
                break
            mu = max(10.0 * mu, 1e-6 * float(np.diag(Hm).max()))
    return dict(T=T, energies=energies, n=n, iterations=it, H=Hm)


# ---- analytic maps of a textured plane (ray-plane intersection, no rasteriser) ----------------------------------------------------------
def texture(x, y):
    """a smooth colour on the plane z = 0, (..., 3) in [0.1, 0.9]"""
    return np.stack([0.5 + 0.4 * np.sin(3.1 * x + 0.3) * np.cos(2.3 * y), 0.5 + 0.4 * np.cos(2.7 * x - 1.1 * y + 0.5),
                     0.5 + 0.4 * np.sin(1.9 * y + 0.8) * np.sin(2.2 * x + 1.7 * y)], -1)


def look_at(eye, at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """world -> camera 4 x 4 of a camera at ``eye`` looking at ``at`` (+z forward, +y down)"""
    eye, at, up = (np.asarray(a, np.float64) for a in (eye, at, up))
    f = at - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = R, -R @ eye
    return V


def plane_cameras(width=48, height=36, focal=None):
    focal = 1.1 * width if focal is None else focal
    out = []
    for k, eye in enumerate(((0.5, -0.3, -2.4), (-0.7, 0.4, -2.2))):
        out.append(dict(viewmat=look_at(eye), fx=focal, fy=focal, cx=width / 2, cy=height / 2, width=width, height=height, image_name=f"cam{k}"))
    return out


def plane_maps(cam, T=np.eye(4), float32=True):
    """the maps of the textured plane z = 0 moved by ``T``, seen from ``cam``: every pixel's ray meets the moved plane; colour from the
    texture at the point's coordinates BEFORE the move.  Coverage 1 everywhere.  float64 when ``float32`` is False (the finite
    differences of the tests need the smooth function, not its rounding)."""
    V = np.asarray(cam["viewmat"], np.float64) @ np.asarray(T, np.float64)         # model -> camera
    R, t = V[:3, :3], V[:3, 3]
    W, H = cam["width"], cam["height"]
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ray = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], -1)
    n_c = R[:, 2]                                   # the plane's normal in the camera frame; t lies on the plane
    z = (n_c @ t) / (ray @ n_c)
    pm = (ray * z[..., None] - t) @ R               # R' (p - t): the model-frame point
    out = dict(image=texture(pm[..., 0], pm[..., 1]), depth=z, alpha=np.ones_like(z))
    return {k: a.astype(np.float32) for k, a in out.items()} if float32 else out


def plane_start():
    """2 degrees about the plane's normal and (0.06, -0.04, 0) off: the motion no depth map sees"""
    return se3_exp([0.0, 0.0, np.deg2rad(2.0), 0.06, -0.04, 0.0])


# ---- the splat plane of the end-to-end test ----------------------------------------------------------------------------------------------
PLANE_WIDTH = 2.0


def splat_plane(n_side=20, seed=7):
    """``n_side^2`` flat disc splats (degree 0) on a jittered grid over the square of side ``PLANE_WIDTH`` in z = 0, coloured by
    ``texture``: the scene dict of ``raster_model``"""
    rng = np.random.default_rng(seed)
    step = PLANE_WIDTH / n_side
    g = (np.arange(n_side) + 0.5) * step - PLANE_WIDTH / 2
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g))
    n = x.size
    x = x + rng.uniform(-0.25, 0.25, n) * step
    y = y + rng.uniform(-0.25, 0.25, n) * step
    s = rng.uniform(0.55, 0.75, n) * step
    cov6 = np.zeros((n, 6))
    cov6[:, 0], cov6[:, 3], cov6[:, 5] = s * s, s * s, (0.02 * step) ** 2
    C0 = 0.28209479177387814
    return dict(xyz=np.stack([x, y, np.zeros(n)], 1).astype(np.float32), cov6=cov6.astype(np.float32), opacity=np.full(n, 4.0, np.float32),
                color=((texture(x, y) - 0.5) / C0).astype(np.float32), sh=np.zeros((n, 0), np.float32), sh_degree=0)


def splat_start():
    """2 degrees about the normal and 3 % of the plane's width along both in-plane axes"""
    return se3_exp([0.0, 0.0, np.deg2rad(2.0), 0.03 * PLANE_WIDTH, -0.03 * PLANE_WIDTH * 0.5, 0.0])


def pose_error(T, T_true=np.eye(4)):
    """(translation error, rotation error in radians) of ``T`` against ``T_true``; the angle from the skew part (exact for small angles,
    where an arccos of the trace rounds to 0)"""
    D = np.asarray(T, np.float64) @ np.linalg.inv(T_true)
    S = D[:3, :3] - D[:3, :3].T
    s = 0.5 * np.linalg.norm([S[2, 1], S[0, 2], S[1, 0]])
    c = (np.trace(D[:3, :3]) - 1) / 2
    return float(np.linalg.norm(D[:3, 3])), float(np.arctan2(s, c))


E2E = dict(width=96, height=72, scales=(4, 2, 1), max_depth_diff=0.5, max_iteration=20, min_increment=1e-6)


def scaled_camera(cam, s):
    return dict(cam, fx=cam["fx"] / s, fy=cam["fy"] / s, cx=cam["cx"] / s, cy=cam["cy"] / s, width=max(1, cam["width"] // s), height=max(1, cam["height"] // s))


def refine_splat_plane(dtype=np.float64):
    """the end-to-end case on the CPU: ``splat_plane`` against itself from ``splat_start``, the project's NumPy renderer
    (``raster_aux_model.render_aux`` in ``dtype``, no radius clip) and this module's loop, level by level
    -> dict(T, energy_initial, energy_final, levels)"""
    import raster_aux_model as A
    scene = splat_plane()
    cams = plane_cameras(E2E["width"], E2E["height"])

    def maps(cam, T=np.eye(4)):
        r = A.render_aux(scene, dict(cam, viewmat=(np.asarray(cam["viewmat"], np.float64) @ T).astype(np.float32)), dtype=dtype, radius_clip=0.0)
        return {k: r[k].astype(np.float32) for k in ("image", "depth", "alpha")}
    T, levels = splat_start(), []
    for s in E2E["scales"]:
        lc = [scaled_camera(c, s) for c in cams]
        r = refine(maps, [maps(c) for c in lc], lc, T, max_depth_diff=E2E["max_depth_diff"], max_iteration=E2E["max_iteration"],
                   min_increment=E2E["min_increment"])
        T = r["T"]
        levels.append(dict(scale=s, iterations=r["iterations"], energies=r["energies"], n=r["n"]))
    return dict(T=T, levels=levels)


GOLDEN_E2E = "photo_refine_expected.json"


def e2e_expected():
    """what ``tests/golden/photo_refine_expected.json`` holds: the errors of the float64 run (``python tests/photo_model.py`` writes it)"""
    r = refine_splat_plane()
    t0, r0 = pose_error(splat_start())
    t1, r1 = pose_error(r["T"])
    return dict(initial_translation_error=t0, initial_rotation_error=r0, initial_in_plane_error=float(np.linalg.norm(splat_start()[:2, 3])),
                translation_error=t1, rotation_error=r1, in_plane_error=float(np.linalg.norm(r["T"][:2, 3])),
                energy_initial=r["levels"][0]["energies"][0], energy_final=r["levels"][-1]["energies"][-1],
                iterations=[lv["iterations"] for lv in r["levels"]], n_pixels=[int(lv["n"]) for lv in r["levels"]], settings={k: list(v) if isinstance(v, tuple) else v for k, v in E2E.items()})


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_E2E)
    with open(path, "w") as f:
        json.dump(e2e_expected(), f, indent=1)
    print(open(path).read())
