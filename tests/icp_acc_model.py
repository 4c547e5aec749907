"""Float64 NumPy model of one ICP evaluation: the 32 accumulator slots that icp_rows (csrc/icp.hip) fills, for every estimator and every
robust loss, for tests/test_icp_acc_cpu.py and tests/test_icp_acc_gpu.py.  No GPU and no call into the library.

Everything is written from the definitions, not from the kernel:

  correspondences   p = T float64(src32); nearest target point by scipy's cKDTree on the float64 target; accepted iff d^2 < max_corr^2.
  a residual row    r(p) is affine in p with gradient g = dr/dp.  A small rigid motion moves p by w x p + t (w = the three angles of
                    Rz(x2) Ry(x1) Rx(x0) at x = 0, t = x3..5), so dr = g . (w x p + t) = (p x g) . w + g . t:   J = [p x g, g].
                      point-to-plane   r = (p - q) . n,                                    g = n
                      generalized      r_i = W_i . (p - q), W = (Ct + R Cs R^T)^(-1/2),    g = W_i      (three rows, W held fixed)
                      coloured         geometric: sqrt(lambda) times the point-to-plane row;
                                       photometric (Open3D TransformationEstimationForColoredICP): the target's intensity is
                                       continued over its tangent plane, I(p) = It + dIt . (proj(p) - q), proj(p) = p - ((p - q) . n) n,
                                       r = sqrt(1 - lambda) (Is - I(p)),                   g = -sqrt(1 - lambda) (I - n n^T) dIt
  a robust loss     is its rho(r); the weight of a row is w = rho'(r) / r in closed form (rho and weight below, checked against each
                    other by finite differences in test_icp_acc_cpu.py).
  the slots         0 count, 1 sum d^2; kinds 0 / 4: 2..16 = sum a, sum b, sum a b^T (row-major), a = p - ctr, b = q - ctr, kind 4 adds
                    17 = sum |a|^2; kinds 1..3: 2..22 the upper triangle of sum J^T w J row by row, 23..28 sum J^T w r, 29 the
                    unweighted sum r^2.  Entries at and past NACC are zero.

`abs` (per slot, the sum of |term|) is the scale every bound is stated in, `terms` the number of terms of the slot.
"""
import functools
import json
import math
import os

import numpy as np
from scipy.spatial import cKDTree

L2, TUKEY, CAUCHY, GM, HUBER = 0, 1, 2, 3, 4
LOSSES = (L2, TUKEY, CAUCHY, GM, HUBER)
LOSS_NAME = {L2: "L2", TUKEY: "Tukey", CAUCHY: "Cauchy", GM: "GM", HUBER: "Huber"}
K = {L2: 0.0, TUKEY: 0.01, CAUCHY: 0.01, GM: 1e-4, HUBER: 0.01}          # the k of each loss in every scene
SWITCHED = (TUKEY, HUBER)                                                 # the losses whose weight has a branch at |r| = k
KINDS = (0, 1, 2, 3, 4)
NACC = {0: 17, 4: 18, 1: 30, 2: 30, 3: 30}
ROWS = {0: 0, 4: 0, 1: 1, 2: 3, 3: 2}                                     # residual rows per matched pair
ACC_LEN = 32
TINY = 1e-300
EPS53 = 2.0 ** -53
TOLERANCE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_acc_tolerance.json")


# -------------------------------------------------------------------------------------------------------------------- losses
def rho(loss, k, r):
    """The loss itself, rho(r) (scalar or array)."""
    r = np.asarray(r, np.float64)
    if loss == L2:
        return 0.5 * r * r
    if loss == HUBER:                       # quadratic inside k, linear outside, C1 at k
        return np.where(np.abs(r) <= k, 0.5 * r * r, k * (np.abs(r) - 0.5 * k))
    if loss == TUKEY:                       # the biweight: saturates at k^2 / 6
        u = np.minimum(np.abs(r) / k, 1.0)
        return k * k / 6.0 * (1.0 - (1.0 - u * u) ** 3)
    if loss == CAUCHY:
        return 0.5 * k * k * np.log1p((r / k) ** 2)
    if loss == GM:                          # Geman-McClure in Open3D's form: k is the squared scale
        return 0.5 * r * r / (k + r * r)
    raise ValueError(loss)


def weight(loss, k, r):
    """w(r) = rho'(r) / r in closed form (its limit at r = 0)."""
    r = np.asarray(r, np.float64)
    if loss == L2:
        return np.ones_like(r)
    if loss == HUBER:                       # rho' = r | k sign(r)
        return np.where(np.abs(r) <= k, 1.0, k / np.maximum(np.abs(r), TINY))
    if loss == TUKEY:                       # rho' = r (1 - (r / k)^2)^2 | 0
        u = np.abs(r) / k
        return np.where(u <= 1.0, (1.0 - u * u) ** 2, 0.0)
    if loss == CAUCHY:                      # rho' = r / (1 + (r / k)^2)
        return 1.0 / (1.0 + (r / k) ** 2)
    if loss == GM:                          # rho' = r k / (k + r^2)^2
        return k / (k + r * r) ** 2
    raise ValueError(loss)


# --------------------------------------------------------------------------------------------------------------------- pieces
def full_cov(c):
    """(N, 6) [xx xy xz yy yz zz] or (N, 3, 3) -> (N, 3, 3) float64"""
    c = np.asarray(c, np.float64)
    return c if c.ndim == 3 else c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def euler6(x):
    """4x4 of the 6-DoF step x: rotation Rz(x2) Ry(x1) Rx(x0), translation x3..5."""
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx
    M[:3, 3] = x[3:6]
    return M


def rigid(deg, axis, t):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    th = math.radians(deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    T[:3, 3] = t
    return T


def moved(T, x):
    """p = T x, every coordinate as the float64 expression ((T0 x + T1 y) + T2 z) + T3 evaluated left to right without fused
    multiply-adds (a BLAS product may fuse and reassociate; the library is compiled with -ffp-contract=off)"""
    T = np.asarray(T, np.float64)
    return np.stack([((T[a, 0] * x[:, 0] + T[a, 1] * x[:, 1]) + T[a, 2] * x[:, 2]) + T[a, 3] for a in range(3)], axis=1)


def sqdist(p, q):
    d = p - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def gicp_w(T, cs, ct):
    """W = (Ct + R Cs R^T)^(-1/2) per pair by numpy.linalg.eigh, and the condition number of each sum."""
    R = T[:3, :3]
    M = ct + R @ cs @ R.T
    lam, V = np.linalg.eigh(M)
    W = (V / np.sqrt(lam)[:, None, :]) @ np.swapaxes(V, 1, 2)
    return W, lam[:, 2] / lam[:, 0]


def residual_rows(kind, T, p, q, jm, im, *, normals=None, src_cov=None, tgt_cov=None, src_int=None, tgt_int=None, tgt_grad=None,
                  lambda_geometric=0.968):
    """The rows of the matched pairs (p, q: (m, 3); jm / im: their target / source indices): g (m, rows, 3) and r (m, rows), and
    the condition numbers of the generalized kind's covariance sums (else None).  J = [p x g, g]."""
    d = p - q
    cond = None
    if kind == 1:
        g = np.asarray(normals, np.float64)[jm][:, None, :]
    elif kind == 2:
        g, cond = gicp_w(T, full_cov(src_cov)[im], full_cov(tgt_cov)[jm])
    elif kind == 3:
        n = np.asarray(normals, np.float64)[jm]
        dit = np.asarray(tgt_grad, np.float64)[jm]
        sg, sp = math.sqrt(lambda_geometric), math.sqrt(1.0 - lambda_geometric)
        gp = -sp * (dit - (dit * n).sum(1)[:, None] * n)                    # -sqrt(1 - lambda) (I - n n^T) dIt
        g = np.stack([sg * n, gp], axis=1)
    else:
        raise ValueError(kind)
    r = np.einsum("mrc,mc->mr", g, d)
    if kind == 3:                                                           # the photometric row is affine, not linear, in p - q
        proj = d - (d * n).sum(1)[:, None] * n                              # proj(p) - q
        it = np.asarray(tgt_int, np.float64)[jm] + (dit * proj).sum(1)
        r[:, 1] = sp * (np.asarray(src_int, np.float64)[im] - it)
    return g, r, cond


def jacobian(p, g):
    """J = [p x g, g] per row: (m, rows, 6)"""
    return np.concatenate([np.cross(p[:, None, :], g), g], axis=2)


UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def model(src32, tgt32, T, max_corr, kind, loss, k, *, normals=None, src_cov=None, tgt_cov=None, src_int=None, tgt_int=None,
          tgt_grad=None, lambda_geometric=0.968, centre=None):
    """One evaluation at T.  Returns a dict:
      acc, abs, terms       (32,) float64 / float64 / int64, the library's slot layout
      matched               (ns,) bool;  j (ns,) int64, the target index or -1;  d2 (ns,) the squared distance to the nearest target
      p                     (ns, 3) the moved source
      margin_tie            min over the source of (second nearest d^2 - nearest d^2) / nearest-second d^2 (inf with one target point)
      margin_corr           min |d^2 - max_corr^2| / max_corr^2
      margin_k              min | |r| - k | / k over every row (inf when the loss has no k or the kind no rows)
      below_k               the fraction of the rows with |r| < k (nan likewise)
      cond                  the largest condition number of Ct + R Cs R^T (kind 2, else 0)
      J, r, w               the rows themselves, (rows_total, 6), (rows_total,), (rows_total,)  (kinds 1..3)"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    src = np.asarray(src32, np.float32).astype(np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt32, np.float32).astype(np.float64).reshape(-1, 3)
    ns = len(src)
    p = moved(T, src)
    kk = min(2, len(tgt))
    dist, jj = cKDTree(tgt).query(p, k=kk)
    dist, jj = dist.reshape(ns, kk), jj.reshape(ns, kk)
    j1 = jj[:, 0]
    d2 = sqdist(p, tgt[j1])                                # the squared distance itself, not the square of a rounded root
    mc2 = max_corr * max_corr
    m = d2 < mc2
    out = {"p": p, "matched": m, "j": np.where(m, j1, -1).astype(np.int64), "d2": d2, "cond": 0.0}
    if kk == 2:
        d2b = sqdist(p, tgt[jj[:, 1]])
        out["margin_tie"] = float(((d2b - d2) / np.maximum(d2b, TINY)).min()) if ns else math.inf
    else:
        out["margin_tie"] = math.inf
    out["margin_corr"] = float((np.abs(d2 - mc2) / mc2).min()) if ns else math.inf
    acc, ab, terms = np.zeros(ACC_LEN), np.zeros(ACC_LEN), np.zeros(ACC_LEN, np.int64)
    nm = int(m.sum())
    im, jm = np.nonzero(m)[0], j1[m]
    pm, qm = p[m], tgt[jm]
    acc[0] = ab[0] = nm
    acc[1] = ab[1] = d2[m].sum()
    terms[:2] = nm
    out.update(margin_k=math.inf, below_k=math.nan, J=np.zeros((0, 6)), r=np.zeros(0), w=np.zeros(0))
    if kind in (0, 4):
        ctr = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
        a, b = pm - ctr, qm - ctr
        cols = [a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]] + [a[:, i] * b[:, j] for i in range(3) for j in range(3)]
        if kind == 4:
            cols.append((a * a).sum(1))
        for s, c in enumerate(cols):
            acc[2 + s], ab[2 + s] = c.sum(), np.abs(c).sum()
        terms[2:NACC[kind]] = nm
    else:
        g, r, cond = residual_rows(kind, T, pm, qm, jm, im, normals=normals, src_cov=src_cov, tgt_cov=tgt_cov, src_int=src_int,
                                   tgt_int=tgt_int, tgt_grad=tgt_grad, lambda_geometric=lambda_geometric)
        J = jacobian(pm, g).reshape(-1, 6)
        r = r.reshape(-1)
        w = weight(loss, k, r)
        for s, (a, b) in enumerate(UPPER):
            c = J[:, a] * w * J[:, b]
            acc[2 + s], ab[2 + s] = c.sum(), np.abs(c).sum()
        for a in range(6):
            c = J[:, a] * w * r
            acc[23 + a], ab[23 + a] = c.sum(), np.abs(c).sum()
        acc[29] = ab[29] = (r * r).sum()
        terms[2:30] = len(r)
        out.update(J=J, r=r, w=w, cond=float(cond.max()) if cond is not None and len(cond) else 0.0)
        if loss in SWITCHED and len(r):
            out["margin_k"] = float((np.abs(np.abs(r) - k) / k).min())
            out["below_k"] = float((np.abs(r) < k).mean())
    out.update(acc=acc, abs=ab, terms=terms)
    return out


def slot_bound(res, cost):
    """Per slot: (terms + 32) 2^-53 abs, the reordering bound of a float64 sum of `terms` values, + 4 cost abs, four times what
    float64 costs the model itself (tests/golden/icp_acc_tolerance.json; 0 for kinds 0 and 4)."""
    return (res["terms"] + 32) * EPS53 * res["abs"] + 4.0 * cost * res["abs"]


# --------------------------------------------------------------------------------------------------------------------- update
def update(acc, kind, centre=None):
    """The estimator's update from the 32 slots.  Kinds 0 / 4: Umeyama (mean-free cross-covariance of q against p, numpy.linalg.svd,
    the reflection guard, with the scale sum(s D) / var(p) for kind 4).  Kinds 1..3: x = solve(JTJ, -JTr), then the Euler matrix.
    No correspondence: the identity."""
    acc = np.asarray(acc, np.float64)
    n = acc[0]
    if not n > 0:
        return np.eye(4)
    if kind in (0, 4):
        ctr = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
        ma, mb = acc[2:5] / n, acc[5:8] / n
        S = acc[8:17].reshape(3, 3).T / n - np.outer(mb, ma)               # E[b a^T] - E[b] E[a]^T
        U, s, Vt = np.linalg.svd(S)
        D = np.ones(3)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0:
            D[2] = -1.0
        R = U @ np.diag(D) @ Vt
        if kind == 4:
            var = acc[17] / n - ma @ ma
            c = (s * D).sum() / var if var > 0 else 0.0
            if not c > 0:
                return np.eye(4)
            R = c * R
        M = np.eye(4)
        M[:3, :3] = R
        M[:3, 3] = mb + ctr - R @ (ma + ctr)
        return M
    A, b = normal_equations(acc)
    return euler6(np.linalg.solve(A, b))


def normal_equations(acc):
    A = np.zeros((6, 6))
    for s, (a, b) in enumerate(UPPER):
        A[a, b] = A[b, a] = acc[2 + s]
    return A, -np.asarray(acc[23:29], np.float64)


def update_bound(acc, bound, kind, centre=None):
    """Per entry of the 4x4 update: what the slot bounds allow it to move, to first order, times 4.
    Kinds 1..3: |dx| <= |A^-1| (|db| + |dA| |x|) in the 2-norm (dA, db = the slot bounds, dA in the Frobenius norm); every entry of
    the rotation is a product of sines and cosines of the three angles, so it moves by at most |dx0| + |dx1| + |dx2| <= sqrt(3) |dx|,
    a translation entry by at most |dx|.
    Kinds 0 / 4: the update is differentiated slot by slot, (update(acc + bound_s e_s) - update(acc - bound_s e_s)) / 2, and the
    absolute values are added over the slots."""
    out = np.zeros((4, 4))
    if kind in (0, 4):
        for s in range(2, NACC[kind]):
            if bound[s] > 0:
                e = np.zeros(ACC_LEN)
                e[s] = bound[s]
                out += np.abs(update(acc + e, kind, centre) - update(acc - e, kind, centre)) / 2.0
        return 4.0 * out
    A, b = normal_equations(acc)
    dA, db = normal_equations(bound)
    x = np.linalg.solve(A, b)
    dx = np.linalg.norm(np.linalg.inv(A), 2) * (np.linalg.norm(db) + np.linalg.norm(dA, "fro") * np.linalg.norm(x))
    out[:3, :3] = math.sqrt(3.0) * dx
    out[:3, 3] = dx
    return 4.0 * out


def step_bound(acc, bound, kind, T, centre=None):
    """Per entry of T1 = update T: |d update| |T|."""
    return update_bound(acc, bound, kind, centre) @ np.abs(np.asarray(T, np.float64))


# --------------------------------------------------------------------------------------------------------------------- scenes
NT = 2000
NS = (1, 63, 257, 3001)
MAX_CORR = (0.03, 0.25)
SCENES = [(ns, mc) for mc in MAX_CORR for ns in NS]
T0 = rigid(5.0, (0.2, 1.0, -0.3), (0.05, -0.02, 0.03))
LAMBDA = 0.5          # lambda_geometric of the scenes: with the default 0.968 the photometric rows (colour noise 2 %) all lie below k = 0.01
# Where the source points that sit near no target point are drawn: max_corr 0.03 -> anywhere in the unit box, as in
# test_sim3_gpu.py::test_accumulate_slots (a fifth of them still meets a target point within 0.03).  At max_corr 0.25 EVERY point of the
# unit box has a target point within reach (2 000 points: the mean spacing is 0.08), and the matched fraction would be 1; there they are
# drawn in the box grown by 1 on every side, [-1, 2]^3, of which an eighth lies within 0.25 of the target -- the matched fraction stays
# between 0.4 and 0.7, and the queries beyond the grid (clamped cells, the early leave of icp_nearest) are part of the scene.
FAR_GROW = {0.03: 0.0, 0.25: 1.0}


def _field(x):
    """a smooth colour field of position, (n, 3) in [0.2, 0.8], and its analytic gradient of the mean channel"""
    f = np.array([[1.3, 0.4, -0.7], [-0.5, 1.1, 0.8], [0.6, -0.9, 1.2]])
    ph = np.array([0.3, 1.1, 2.0])
    arg = x @ f.T + ph
    rgb = 0.5 + 0.3 * np.sin(arg)
    grad = (0.3 * np.cos(arg))[:, :, None] * f[None, :, :]
    return rgb, grad.mean(1)


def _spd(rng, n):
    """n float64 SPD covariances whose axes (standard deviations) lie between 0.4 / sqrt(30) and 0.4 sqrt(30): axis ratios up to 30,
    and a scale at which the whitened residuals W (p - q) of offsets of 0.01 straddle k = 0.01"""
    h = 0.5 * math.log(30.0)
    ax = 0.4 * np.exp(rng.uniform(-h, h, size=(n, 3)))
    Q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    C = (Q * (ax * ax)[:, None, :]) @ np.swapaxes(Q, 1, 2)
    return 0.5 * (C + np.swapaxes(C, 1, 2))


def six(C):
    return np.ascontiguousarray(C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])


@functools.lru_cache(maxsize=None)
def target():
    rng = np.random.default_rng(2000)
    xyz = rng.random((NT, 3)).astype(np.float32)
    nrm = rng.normal(size=(NT, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rgb, grad = _field(xyz.astype(np.float64))
    rgb = rgb + 0.02 * rng.normal(size=rgb.shape)
    tangent = grad - (grad * nrm).sum(1)[:, None] * nrm          # a stand-in for the library's estimated gradient, for the CPU tests
    return {"xyz": xyz, "normals": nrm, "cov": six(_spd(rng, NT)), "rgb": rgb, "int": rgb.sum(1) / 3.0, "grad": tangent}


@functools.lru_cache(maxsize=None)
def scene(ns, max_corr):
    """The seeded pair (ns source points, the 2 000-point target) at T0; the arrays are shared: do not write to them."""
    tg = target()
    rng = np.random.default_rng(100 + ns)
    moved = tg["xyz"][rng.integers(0, NT, ns)].astype(np.float64) + 0.01 * rng.normal(size=(ns, 3))
    far = np.arange(ns) % 2 == 1
    g = FAR_GROW[max_corr]
    moved[far] = rng.random((int(far.sum()), 3)) * (1.0 + 2.0 * g) - g
    src = ((moved - T0[:3, 3]) @ np.linalg.inv(T0[:3, :3]).T).astype(np.float32)
    rgb, _ = _field(moved)
    rgb = rgb + 0.02 * rng.normal(size=rgb.shape)
    return {"name": f"ns{ns}_mc{max_corr}", "ns": ns, "max_corr": max_corr, "T": T0, "src": src, "tgt": tg["xyz"], "normals": tg["normals"],
            "tgt_cov": tg["cov"], "src_cov": six(_spd(rng, ns)), "tgt_rgb": tg["rgb"], "src_rgb": rgb, "tgt_int": tg["int"],
            "src_int": rgb.sum(1) / 3.0, "grad": tg["grad"]}


def scene_model(sc, kind, loss, T=None, *, tgt_grad=None, centre=None, rows=None):
    """model() on a scene (`rows`: only these source rows)."""
    sel = slice(None) if rows is None else rows
    return model(sc["src"][sel], sc["tgt"], sc["T"] if T is None else T, sc["max_corr"], kind, loss, K[loss], normals=sc["normals"],
                 src_cov=sc["src_cov"][sel], tgt_cov=sc["tgt_cov"], src_int=sc["src_int"][sel], tgt_int=sc["tgt_int"],
                 tgt_grad=sc["grad"] if tgt_grad is None else tgt_grad, lambda_geometric=LAMBDA, centre=centre)


# ------------------------------------------------------------------------------------------- what float64 costs the model itself
HP_PAIRS = 300          # the high-precision model takes the first 300 matched pairs of a scene: the cost is a per-term figure


def model_hp(sc, kind, rows, digits=50):
    """The same model on the source rows `rows` (all matched) in `digits`-digit arithmetic (mpmath): W by mpmath's symmetric
    eigen-solver, every term and every sum.  -> {loss: 32 mpf sums}"""
    import mpmath as mp
    f = mp.mpf
    with mp.workdps(digits):
        T = [[f(float(v)) for v in row] for row in sc["T"]]
        sg, sp = mp.sqrt(f(LAMBDA)), mp.sqrt(1 - f(LAMBDA))
        res = scene_model(sc, kind, L2, rows=rows)
        assert res["matched"].all()
        acc = {loss: [f(0)] * ACC_LEN for loss in LOSSES}

        def vec(a):
            return [f(float(v)) for v in a]

        def dot(a, b):
            return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

        def cross(a, b):
            return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

        def w_of(loss, k, r):
            k = f(k)
            if loss == L2:
                return f(1)
            if loss == HUBER:
                return f(1) if abs(r) <= k else k / abs(r)
            if loss == TUKEY:
                return (1 - (r / k) ** 2) ** 2 if abs(r) <= k else f(0)
            if loss == CAUCHY:
                return 1 / (1 + (r / k) ** 2)
            return k / (k + r * r) ** 2

        for i, j in zip(rows, res["j"]):
            x = vec(sc["src"][i].astype(np.float64))
            q = vec(sc["tgt"][j].astype(np.float64))
            p = [dot(T[a][:3], x) + T[a][3] for a in range(3)]
            d = [p[a] - q[a] for a in range(3)]
            gs, rs = [], []
            if kind in (1, 3):
                n = vec(sc["normals"][j])
            if kind == 1:
                gs, rs = [n], [dot(d, n)]
            elif kind == 2:
                Cs, Ct = full_cov(sc["src_cov"][i:i + 1])[0], full_cov(sc["tgt_cov"][j:j + 1])[0]
                R = mp.matrix([row[:3] for row in T[:3]])
                M = mp.matrix(Ct.tolist()) + R * mp.matrix(Cs.tolist()) * R.T
                E, Q = mp.eigsy(M)
                W = Q * mp.diag([1 / mp.sqrt(E[a]) for a in range(3)]) * Q.T
                for a in range(3):
                    g = [W[a, 0], W[a, 1], W[a, 2]]
                    gs.append(g)
                    rs.append(dot(g, d))
            elif kind == 3:
                dit = vec(sc["grad"][j])
                dn = dot(d, n)
                proj = [d[a] - dn * n[a] for a in range(3)]
                ditn = dot(dit, n)
                gs = [[sg * n[a] for a in range(3)], [-sp * (dit[a] - ditn * n[a]) for a in range(3)]]
                rs = [sg * dn, sp * (f(float(sc["src_int"][i])) - (f(float(sc["tgt_int"][j])) + dot(dit, proj)))]
            d2 = dot(d, d)
            for g, r in zip(gs, rs):
                J = cross(p, g) + g
                for loss in LOSSES:
                    a_ = acc[loss]
                    w = w_of(loss, K[loss], r)
                    wJ = [w * v for v in J]
                    for s, (a, b) in enumerate(UPPER):
                        a_[2 + s] += J[a] * wJ[b]
                    for a in range(6):
                        a_[23 + a] += wJ[a] * r
                    a_[29] += r * r
            for loss in LOSSES:
                acc[loss][0] += 1
                acc[loss][1] += d2
        return acc


def model_cost(sc, kind):
    """max over the losses and the slots of |acc64 - acc_hp| / (abs + tiny) on the first HP_PAIRS matched pairs; 0 for kinds 0 and 4
    (their terms are single products of the same float64 operands the kernel multiplies)."""
    if kind in (0, 4):
        return 0.0
    import mpmath as mp
    rows = np.nonzero(scene_model(sc, kind, L2)["matched"])[0][:HP_PAIRS]
    if len(rows) == 0:
        return 0.0
    hp = model_hp(sc, kind, rows)
    worst = 0.0
    with mp.workdps(50):
        for loss in LOSSES:
            res = scene_model(sc, kind, loss, rows=rows)
            for s in range(1, NACC[kind]):
                worst = max(worst, float(abs(mp.mpf(float(res["acc"][s])) - hp[loss][s]) / (mp.mpf(float(res["abs"][s])) + mp.mpf(TINY))))
    return worst


def tolerances():
    return {f"{sc['name']}_kind{kind}": model_cost(sc, kind) for sc in (scene(*s) for s in SCENES) for kind in KINDS}


def load_tolerances():
    with open(TOLERANCE_JSON) as fh:
        return json.load(fh)
