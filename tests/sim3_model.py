"""Float64 NumPy / SciPy restatement of the similarity (scaled) registration paths, for tests/test_sim3_cpu.py and
tests/test_sim3_gpu.py: Umeyama with and without scaling, the registration_icp loop with the scaled point-to-point update, and a
splat model moved by a similarity.  Written from the definitions in include/gsr_hip.h (Eigen::umeyama, Open3D 0.16
RegistrationICP); Open3D itself is absent, parity with it is unpinned like the rest of the ICP half.
"""
import math

import numpy as np
from scipy.spatial import cKDTree


# ------------------------------------------------------------------------------------------------------------------ Umeyama
def umeyama(p, q, with_scaling=False):
    """Eigen::umeyama(src = p, dst = q, with_scaling) as a 4x4.  Where Eigen divides by zero (source variance 0, or a scale
    that is not positive) the scaled form returns the identity -- the library's stated deviation."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    n = len(p)
    mp, mq = p.mean(0), q.mean(0)
    S = (q - mq).T @ (p - mp) / n
    U, s, Vt = np.linalg.svd(S)
    D = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2] = -1
    R = U @ np.diag(D) @ Vt
    c = 1.0
    if with_scaling:
        var = ((p - mp) ** 2).sum() / n
        if not var > 0:
            return np.eye(4)
        c = float((s * D).sum() / var)
        if not c > 0:
            return np.eye(4)
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mq - c * R @ mp
    return T


def accumulators(p, q, centre, scaled):
    """The 32-slot accumulator row of the point-to-point kinds from matched pairs (p = moved source, q = target): slots 0..16 of
    kind 0, plus slot 17 = sum |a|^2 when ``scaled``; a = p - centre, b = q - centre."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    a, b = p - centre, q - centre
    acc = np.zeros(32)
    acc[0] = len(p)
    acc[1] = ((p - q) ** 2).sum()
    acc[2:5], acc[5:8] = a.sum(0), b.sum(0)
    acc[8:17] = (a[:, :, None] * b[:, None, :]).sum(0).reshape(9)          # acc[8 + 3 r + s] = sum a_r b_s
    if scaled:
        acc[17] = (a * a).sum()
    return acc


def similarity(c, deg, axis, t):
    """4x4 [c R | t], R = rotation by ``deg`` degrees about ``axis``."""
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    th = math.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = t
    return T


def scale_of(T):
    return float(np.cbrt(np.linalg.det(np.asarray(T, np.float64)[:3, :3])))


# ---------------------------------------------------------------------------------------------------------------------- ICP
def icp(src, tgt, init, max_corr, max_iter, with_scaling=True, rel=1e-6):
    """registration_icp with TransformationEstimationPointToPoint(with_scaling): the conventions of the point-to-point model in
    tests/test_icp_oracle.py -- cKDTree 1-NN (the lowest index on a tie: none occurs in generic data), a pair counts iff
    d^2 < max_corr^2 (strict), stop when |d fitness| < rel and |d rmse| < rel -- with the points taken as p = T p0 from the
    accumulated T in every evaluation, as the kernels do.  src / tgt: the float32 coordinates widened to float64.
    Returns (T, fitness, rmse, iterations)."""
    src, tgt = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)
    tree = cKDTree(tgt)
    T = np.asarray(init, np.float64).copy()

    def evaluate(T):
        p = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(p, k=1)
        m = d * d < max_corr * max_corr
        return p, m, j, (m.sum() / len(src) if m.any() else 0.0), (math.sqrt((d[m] ** 2).mean()) if m.any() else 0.0)

    p, m, j, fit, rmse = evaluate(T)
    it = 0
    for it in range(1, max_iter + 1):
        upd = umeyama(p[m], tgt[j[m]], with_scaling) if m.any() else np.eye(4)
        T = upd @ T
        p, m, j, fit2, rmse2 = evaluate(T)
        stop = abs(fit - fit2) < rel and abs(rmse - rmse2) < rel
        fit, rmse = fit2, rmse2
        if stop:
            break
    return T, fit, rmse, it


# ------------------------------------------------------------------------------------------------------------- splat model
def split(T):
    """-> (c, R, t) of a similarity, float64 (no gate: the tests feed valid ones)."""
    T = np.asarray(T, np.float64)
    c = scale_of(T)
    return c, T[:3, :3] / c, T[:3, 3].copy()


def narrowed(T):
    """(c, c^2, ln c, R, t) as the kernel holds them: each narrowed to float32 once from float64, returned as float64."""
    c, R, t = split(T)
    f = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    return float(f(c)), float(f(c * c)), float(f(math.log(c))), f(R), f(t)


def full_cov(c6):
    c = np.asarray(c6, np.float64)
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def six(Cf):
    return Cf[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def model_similarity(T, xyz, cov6, quat, scaling):
    """The moved arrays in float64 with the kernel's float32 constants: xyz' = c (R x) + t, cov' = c^2 (R S R^T), the rotation
    MATRIX of rot' (R R(q), q normalised), scaling' = scaling + ln c.  Returns a dict; 'abs_xyz' / 'abs_cov' are the
    magnitudes |c| |R| |x| + |t| and c^2 |R| |S| |R^T| the error bounds scale with."""
    c, c2, lnc, R, t = narrowed(T)
    x = np.asarray(xyz, np.float64)
    S = full_cov(cov6)
    out = {"xyz": c * (x @ R.T) + t, "abs_xyz": c * (np.abs(x) @ np.abs(R).T) + np.abs(t),
           "cov6": c2 * six(R @ S @ R.T), "abs_cov": c2 * six(np.abs(R) @ np.abs(S) @ np.abs(R).T), "lnc": lnc, "R": split(T)[1]}
    if scaling is not None:
        out["scaling"] = np.asarray(scaling, np.float64) + lnc
    if quat is not None:
        q = np.asarray(quat, np.float64)
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        out["rot_matrix"] = split(T)[1] @ quat_to_rot(q)
    return out


def quat_to_rot(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
