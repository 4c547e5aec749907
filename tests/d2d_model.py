"""Float64 model of mixture-to-mixture registration (the definition is the header comment of include/gsr_hip.h).

Every expression is formed in the order csrc/gsr_d2d.h forms it, from the widened float32 inputs, with separate multiplications and
additions (NumPy never contracts them).  ``exp`` is the C library's (``math.exp``), one call per pair: NumPy's vector ``exp`` is a
different implementation with its own error.  Pairs come from a ``cKDTree`` query with a slightly larger radius and then the
definition's own strict test.  The order of SUMMATION is the model's own (row by row, pairs by target index): the kernel's differs,
and the tests' tolerance is what two orders can differ by.

Also here: the scene of the prototype (a wavy floor plus a wavy wall, sampled twice independently, disc-shaped covariances), and
NumPy restatements of the step, the loop and a point-to-point ICP on the centres.
"""
import math

import numpy as np
from scipy.spatial import cKDTree

SUMS_LEN = 32
_exp = np.frompyfunc(math.exp, 1, 1)


def rigid(angle_deg, axis, shift):
    """4 x 4 of a rotation by ``angle_deg`` about ``axis`` (Rodrigues) and a shift"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = shift
    return T


def _full(c6):
    """(n, 6) xx xy xz yy yz zz -> (n, 3, 3)"""
    return np.stack([np.stack([c6[:, 0], c6[:, 1], c6[:, 2]], -1), np.stack([c6[:, 1], c6[:, 3], c6[:, 4]], -1),
                     np.stack([c6[:, 2], c6[:, 4], c6[:, 5]], -1)], -2)


def move_points(T, p):
    """p' = R p + t, the products of a row added left to right"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([T[a, 0] * x + T[a, 1] * y + T[a, 2] * z + T[a, 3] for a in range(3)], -1)


def rotate_cov(T, A6):
    """S = R A R': G = R A, then S = G R', upper triangle"""
    A = _full(A6)
    G = [[T[a, 0] * A[:, 0, b] + T[a, 1] * A[:, 1, b] + T[a, 2] * A[:, 2, b] for b in range(3)] for a in range(3)]
    return np.stack([G[a][0] * T[b, 0] + G[a][1] * T[b, 1] + G[a][2] * T[b, 2] for a in range(3) for b in range(a, 3)], -1)


def pairs(src_xyz, tgt_xyz, T, max_corr, src_ok, tgt_ok):
    """-> (i, j, p') of every counted pair, sorted by (i, j)"""
    p = move_points(T, src_xyz.astype(np.float64))
    q = tgt_xyz.astype(np.float64)
    si, tj = np.flatnonzero(src_ok), np.flatnonzero(tgt_ok)
    if len(si) == 0 or len(tj) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), p
    tree = cKDTree(q[tj])
    lists = tree.query_ball_point(p[si], max_corr * (1 + 1e-9) + 1e-12)
    I = np.concatenate([np.full(len(l), si[k], np.int64) for k, l in enumerate(lists)] + [np.zeros(0, np.int64)])
    J = np.concatenate([tj[np.asarray(l, np.int64)] for l in lists] + [np.zeros(0, np.int64)])
    r = p[I] - q[J]
    d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
    keep = d2 < max_corr * max_corr
    I, J = I[keep], J[keep]
    o = np.lexsort((J, I))
    return I[o], J[o], p


def finite_rows(xyz, cov6, weight):
    ok = np.isfinite(xyz).all(1) & np.isfinite(cov6).all(1)
    return ok if weight is None else ok & np.isfinite(weight)


def pair_terms(src, tgt, T, max_corr, cov_scale=1.0, cov_floor=0.0):
    """src, tgt = (xyz, cov6, weight or None), float32.  -> dict of the per-pair quantities of the counted, non-singular pairs
    (i, j, p', r, M (n, 6), Mr, m, omega) and ``n_singular``"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    (sx, sA, sw), (tx, tB, tv) = src, tgt
    I, J, p = pairs(sx, tx, T, max_corr, finite_rows(sx, sA, sw), finite_rows(tx, tB, tv))
    S = rotate_cov(T, sA.astype(np.float64))[I]
    B = tB.astype(np.float64)[J]
    r = p[I] - tx.astype(np.float64)[J]
    s2, phi = cov_scale * cov_scale, cov_floor
    C = [s2 * (S[:, k] + B[:, k]) + (phi if k in (0, 3, 5) else 0.0) for k in range(6)]
    # (adding 0.0 to an off-diagonal entry changes nothing but the sign of a zero, which no later product or sum keeps apart)
    a = [C[3] * C[5] - C[4] * C[4], C[2] * C[4] - C[1] * C[5], C[1] * C[4] - C[2] * C[3],
         C[0] * C[5] - C[2] * C[2], C[1] * C[2] - C[0] * C[4], C[0] * C[3] - C[1] * C[1]]
    det = C[0] * a[0] + C[1] * a[1] + C[2] * a[2]
    ok = (det > 0) & np.isfinite(det)
    n_singular = int((~ok).sum())
    I, J, r, det = I[ok], J[ok], r[ok], det[ok]
    inv = 1.0 / det
    M = np.stack([ak[ok] * inv for ak in a], -1)
    Mr = np.stack([M[:, 0] * r[:, 0] + M[:, 1] * r[:, 1] + M[:, 2] * r[:, 2], M[:, 1] * r[:, 0] + M[:, 3] * r[:, 1] + M[:, 4] * r[:, 2],
                   M[:, 2] * r[:, 0] + M[:, 4] * r[:, 1] + M[:, 5] * r[:, 2]], -1)
    m = r[:, 0] * Mr[:, 0] + r[:, 1] * Mr[:, 1] + r[:, 2] * Mr[:, 2]
    w = np.ones(len(sx)) if sw is None else sw.astype(np.float64)
    v = np.ones(len(tx)) if tv is None else tv.astype(np.float64)
    e = _exp(-0.5 * m).astype(np.float64) if len(m) else np.zeros(0)
    omega = (w[I] * v[J]) * e
    return dict(i=I, j=J, p=p, r=r, M=M, Mr=Mr, m=m, omega=omega, n_singular=n_singular, ns=len(sx))


def _cross(p, v):
    return np.stack([p[:, 1] * v[:, 2] - p[:, 2] * v[:, 1], p[:, 2] * v[:, 0] - p[:, 0] * v[:, 2], p[:, 0] * v[:, 1] - p[:, 1] * v[:, 0]], -1)


def _expand(p, W, b):
    """the 27 entries of J' W J and J' b of every row (gsr_d2d.h, row_expand); with the absolute values of p, W and b and ``+`` for
    ``-`` it gives the sum of the magnitudes of the products added"""
    col = [np.stack([W[:, 0], W[:, 1], W[:, 2]], -1), np.stack([W[:, 1], W[:, 3], W[:, 4]], -1), np.stack([W[:, 2], W[:, 4], W[:, 5]], -1)]
    A = np.stack([_cross(p, col[c]) for c in range(3)], -1)             # A[:, a, c]
    Hrr = np.stack([_cross(p, A[:, a, :]) for a in range(3)], -2)       # Hrr[:, a, b]
    out = np.zeros((len(p), 27))
    out[:, 0:3], out[:, 3:6] = Hrr[:, 0, :], A[:, 0, :]
    out[:, 6:8], out[:, 8:11] = Hrr[:, 1, 1:], A[:, 1, :]
    out[:, 11], out[:, 12:15] = Hrr[:, 2, 2], A[:, 2, :]
    out[:, 15:21] = W
    out[:, 21:24], out[:, 24:27] = _cross(p, b), b
    return out


def _expand_abs(p, W, b):
    p = np.abs(p)
    cr = lambda v: np.stack([p[:, 1] * v[:, 2] + p[:, 2] * v[:, 1], p[:, 2] * v[:, 0] + p[:, 0] * v[:, 2], p[:, 0] * v[:, 1] + p[:, 1] * v[:, 0]], -1)
    col = [np.stack([W[:, 0], W[:, 1], W[:, 2]], -1), np.stack([W[:, 1], W[:, 3], W[:, 4]], -1), np.stack([W[:, 2], W[:, 4], W[:, 5]], -1)]
    A = np.stack([cr(col[c]) for c in range(3)], -1)
    Hrr = np.stack([cr(A[:, a, :]) for a in range(3)], -2)
    out = np.zeros((len(p), 27))
    out[:, 0:3], out[:, 3:6] = Hrr[:, 0, :], A[:, 0, :]
    out[:, 6:8], out[:, 8:11] = Hrr[:, 1, 1:], A[:, 1, :]
    out[:, 11], out[:, 12:15] = Hrr[:, 2, 2], A[:, 2, :]
    out[:, 15:21] = W
    out[:, 21:24], out[:, 24:27] = cr(b), b
    return out


def accumulate(src, tgt, T, max_corr, cov_scale=1.0, cov_floor=0.0):
    """-> (sums[32], asum[32]).  asum[k] is sum|term_k|: the magnitudes of what sum k adds under the contract's grouping -- per pair
    omega |M_k| and omega |M r|_k carried through the per-row expansion with every factor in absolute value (so for slots 0..26 it is
    the sum of the magnitudes of the PRODUCTS a row's expansion adds, which is what a last-place difference in a pair's omega or in the
    order of the row's additions is scaled by); the sums themselves for 27 and 28; zero for the counts, which are exact."""
    t = pair_terms(src, tgt, T, max_corr, cov_scale, cov_floor)
    ns = t["ns"]
    W, b, s, sm, cnt = np.zeros((ns, 6)), np.zeros((ns, 3)), np.zeros(ns), np.zeros(ns), np.zeros(ns)
    Wa, ba = np.zeros((ns, 6)), np.zeros((ns, 3))
    om = t["omega"]
    np.add.at(W, t["i"], om[:, None] * t["M"])
    np.add.at(b, t["i"], om[:, None] * t["Mr"])
    np.add.at(Wa, t["i"], np.abs(om[:, None] * t["M"]))
    np.add.at(ba, t["i"], np.abs(om[:, None] * t["Mr"]))
    np.add.at(s, t["i"], om)
    np.add.at(sm, t["i"], om * t["m"])
    np.add.at(cnt, t["i"], 1.0)
    rows = cnt > 0
    sums, asum = np.zeros(SUMS_LEN), np.zeros(SUMS_LEN)
    sums[:27] = _expand(t["p"][rows], W[rows], b[rows]).sum(0)
    asum[:27] = _expand_abs(t["p"][rows], Wa[rows], ba[rows]).sum(0)
    sums[27], sums[28] = s.sum(), sm.sum()
    asum[27], asum[28] = np.abs(om).sum(), np.abs(om * t["m"]).sum()
    sums[29], sums[30], sums[31] = len(om), rows.sum(), t["n_singular"]
    return sums, asum


def score(src, tgt, T, max_corr, cov_scale=1.0, cov_floor=0.0):
    return accumulate(src, tgt, T, max_corr, cov_scale, cov_floor)[0][27]


def unpack(sums):
    """-> (H (6, 6), g (6))"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[:21]
    return H + np.triu(H, 1).T, sums[21:27].copy()


def increment(x):
    """the 4 x 4 of a six-vector: Rz(x2) Ry(x1) Rx(x0), translation x3..5 -- what the ICP step forms"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, x[3]],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa, x[4]],
                     [-sb, cb * sa, cb * ca, x[5]],
                     [0.0, 0.0, 0.0, 1.0]])


def register(src, tgt, init, max_corr, cov_scale=1.0, cov_floor=0.0, relative_score=1e-6, max_iter=30):
    """the loop of gsr_d2d_register -> dict(T, score, fitness, mahalanobis_rmse, iterations, status, scores)"""
    T = np.array(init, np.float64).reshape(4, 4)
    prev, iterations, status, scores, it = None, 0, "max_iteration", [], 0
    while True:
        s, _ = accumulate(src, tgt, T, max_corr, cov_scale, cov_floor)
        scores.append(s[27])
        if s[29] == 0:
            status = "no_pairs"
            break
        if prev is not None and abs(s[27] - prev) <= relative_score * s[27]:
            status = "converged"
            break
        if it >= max_iter:
            break
        H, g = unpack(s)
        x = np.linalg.solve(H, -g)
        T = increment(x) @ T
        prev = s[27]
        iterations += 1
        it += 1
    ns = len(src[0])
    return dict(T=T, score=s[27], fitness=s[30] / ns if ns else 0.0, mahalanobis_rmse=np.sqrt(s[28] / s[27]) if s[27] > 0 else 0.0,
                iterations=iterations, status=status, scores=scores, sums=s)


# ---------------------------------------------------------------------------------------------------------------- the prototype's scene
SIGMA_T, SIGMA_N = 0.04, 0.004
TRUTH = rigid(5.0, (1, 1, 1), (0.05, -0.05, 0.025))


def _surface(n, rng):
    """n points on a wavy floor (z = f(x, y)) and a wavy wall (y = g(x, z)), with unit normals"""
    nf = n // 2
    u, v = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    p, nr = np.zeros((n, 3)), np.zeros((n, 3))
    x, y = u[:nf], v[:nf]                                   # floor
    p[:nf] = np.stack([x, y, 0.08 * np.sin(2.5 * x) * np.cos(2.0 * y)], -1)
    nr[:nf] = np.stack([-0.08 * 2.5 * np.cos(2.5 * x) * np.cos(2.0 * y), 0.08 * 2.0 * np.sin(2.5 * x) * np.sin(2.0 * y), np.ones(nf)], -1)
    x, z = u[nf:], 0.5 * (v[nf:] + 1.0)                     # wall, standing on the floor's far edge
    p[nf:] = np.stack([x, 1.0 + 0.06 * np.sin(3.0 * x + 1.0) * np.cos(2.0 * z), z], -1)
    nr[nf:] = np.stack([-0.06 * 3.0 * np.cos(3.0 * x + 1.0) * np.cos(2.0 * z), np.ones(n - nf), 0.06 * 2.0 * np.sin(3.0 * x + 1.0) * np.sin(2.0 * z)], -1)
    return p, nr / np.linalg.norm(nr, axis=1, keepdims=True)


def _discs(nr):
    """cov = sigma_t^2 (I - n n') + sigma_n^2 n n' -> (n, 6)"""
    nn = nr[:, :, None] * nr[:, None, :]
    C = SIGMA_T ** 2 * (np.eye(3)[None] - nn) + SIGMA_N ** 2 * nn
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], -1)


def scene(n, seed, truth=TRUTH):
    """two independent samplings of one scene: the target as it is, the source moved by truth^-1 (so ``truth`` registers it).
    -> dict(src=(xyz, cov6, None), tgt=(...), truth) in float32"""
    rng = np.random.default_rng(seed)
    ps, ns_ = _surface(n, rng)
    pt, nt_ = _surface(n, rng)
    Ti = np.linalg.inv(truth)
    ps = ps @ Ti[:3, :3].T + Ti[:3, 3]
    ns_ = ns_ @ Ti[:3, :3].T
    src = (ps.astype(np.float32), _discs(ns_).astype(np.float32), None)
    tgt = (pt.astype(np.float32), _discs(nt_).astype(np.float32), None)
    for a in src[:2] + tgt[:2]:
        a.setflags(write=False)
    return dict(src=src, tgt=tgt, truth=truth)


def pose_error(T, truth):
    """-> (rotation error in degrees, translation error)"""
    D = np.asarray(T) @ np.linalg.inv(truth)
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    return float(np.rad2deg(np.arccos(c))), float(np.linalg.norm(D[:3, 3]))


def icp_point_to_point(src_xyz, tgt_xyz, init, max_corr, max_iter=60, tol=1e-10):
    """point-to-point ICP on the centres: nearest neighbour within max_corr, Kabsch / Umeyama update, until the RMSE stops changing"""
    T = np.array(init, np.float64)
    q = tgt_xyz.astype(np.float64)
    tree = cKDTree(q)
    prev = None
    for _ in range(max_iter):
        p = move_points(T, src_xyz.astype(np.float64))
        d, j = tree.query(p, distance_upper_bound=max_corr)
        ok = np.isfinite(d)
        if ok.sum() < 3:
            break
        a, b = p[ok], q[j[ok]]
        rmse = np.sqrt((d[ok] ** 2).mean())
        ma, mb = a.mean(0), b.mean(0)
        U, _, Vt = np.linalg.svd((b - mb).T @ (a - ma))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = U @ D @ Vt
        dT = np.eye(4)
        dT[:3, :3], dT[:3, 3] = R, mb - R @ ma
        T = dT @ T
        if prev is not None and abs(prev - rmse) < tol:
            break
        prev = rmse
    return T
