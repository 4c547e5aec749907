"""NumPy restatement of Fast Global Registration (test infrastructure, not the product).

Restates Open3D 0.16 FastGlobalRegistration.cpp as recalled (parity-unpinned: Open3D is not part of this project's environment;
DESIGN.md section 12) with the library's counter-based sampler in place of Open3D's random engine: reciprocal feature matches, the
tuple test, normalisation, the graduated-non-convexity optimisation, the way back to the caller's units and the evaluation.  The
sampler, the scene and the feature search come from tests/global_model.py.
"""
from __future__ import annotations

import math

import numpy as np

import global_model as G


def down(n, seed, voxel, T=None):
    """The test scene voxel-down-sampled, with normals from the averaged covariances turned towards the centroid:
    (xyz float32, normals float64), what preprocess_point_cloud hands to FPFH."""
    sc = G.make_scene(n, seed)
    if T is not None:
        sc = G.transform_scene(sc, T)
    P, C = G.voxel_down(sc["xyz"], sc["cov6"], voxel)
    N = G.normals_from_cov(C)
    c = P.mean(0)
    N = np.where(((c - P) * N).sum(1, keepdims=True) < 0, -N, N)
    return P.astype(np.float32), N


def reciprocal(fs, ft):
    """(corres (m, 2) int64, nn_st, nn_ts): the pairs (i, nn_st[i]) with nn_ts[nn_st[i]] == i, ascending i; no fall-back."""
    nst, nts = G.nn_rows(fs, ft), G.nn_rows(ft, fs)
    i = np.arange(len(fs))
    keep = nts[nst] == i
    return np.stack([i[keep], nst[keep]], 1), nst, nts


def _edge(X, a, b):
    d = X[a] - X[b]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def tuple_test(src_xyz, tgt_xyz, corres, tuple_scale=0.95, maximum_tuple_count=1000, seed=0, chunk=None):
    """(pairs (3 * accepted, 2), n_trials): Open3D's serial loop over trials k = 0 .. 100 m - 1, evaluated `chunk` trials at a time
    only for speed.  n_trials = trials the serial loop visits."""
    P = np.asarray(src_xyz, np.float32).astype(np.float64)
    Q = np.asarray(tgt_xyz, np.float32).astype(np.float64)
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    m = len(corres)
    total = 100 * m
    out = np.zeros((0, 2), np.int64)
    if m == 0 or maximum_tuple_count <= 0:
        return out, 0
    chunk = chunk or total
    taken, k, picked = 0, 0, []
    s = float(tuple_scale)
    while k < total and taken < maximum_tuple_count:
        nb = min(chunk, total - k)
        r = G.ransac_sample(seed, k, nb, m, 3)
        i, j = corres[r, 0], corres[r, 1]
        ok = np.ones(nb, bool)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            li, lj = _edge(P, i[:, a], i[:, b]), _edge(Q, j[:, a], j[:, b])
            with np.errstate(divide="ignore", invalid="ignore"):
                ok &= (li * s < lj) & (lj < li / s)
        acc = np.flatnonzero(ok)[: maximum_tuple_count - taken]
        picked.append(np.stack([i[acc].reshape(-1), j[acc].reshape(-1)], 1))
        taken += len(acc)
        if taken >= maximum_tuple_count:
            return np.vstack(picked), k + int(acc[-1]) + 1
        k += nb
    return np.vstack(picked), total


_tuple_test = tuple_test          # fgr() below has an option of the same name


def fixed_order_mean(X, block=256, max_blocks=256):
    """Mean of the rows of X (n, 3) float64 with the sums taken in the library's fixed order (include/gsr_hip.h: "a fixed order"):
    G = min(ceil(n / 256), 256) blocks of 256 threads; thread t of block b adds the rows b * 256 + t, + G * 256, ... in ascending
    order; the 64 lanes of a wave fold by halves (lane l += lane l + 32, 16, ..., 1); the 4 waves, then the G blocks, in index
    order.  (Adding the zero padding of absent rows changes no bit.)"""
    n = len(X)
    g = min(max((n + block - 1) // block, 1), max_blocks)
    rounds = (n + g * block - 1) // (g * block)
    pad = np.zeros((rounds * g * block, X.shape[1]))
    pad[:n] = X
    pad = pad.reshape(rounds, g, block // 64, 64, X.shape[1])
    v = np.zeros(pad.shape[1:])
    for r in range(rounds):
        v = v + pad[r]
    o = 32
    while o > 0:
        v = v[:, :, :o] + v[:, :, o:2 * o]
        o //= 2
    v = v[:, :, 0]                                    # (g, waves, cols)
    w = np.zeros((g, X.shape[1]))
    for k in range(v.shape[1]):
        w = w + v[:, k]
    s = np.zeros(X.shape[1])
    for b in range(g):
        s = s + w[b]
    return s / float(n)


def solve6_ldlt(A, b):
    """x = A^-1 b by LDL^T with diagonal pivoting (largest |diagonal|, first on ties), the elimination of csrc/gsr_solve.h; None when
    the solution is not finite (zero or non-finite pivot)."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = 6
    L = np.zeros((n, n))
    D = np.zeros(n)
    perm = list(range(n))
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = k + int(np.argmax(np.abs(np.diag(A)[k:])))
            if piv != k:
                A[[k, piv], :] = A[[piv, k], :]
                A[:, [k, piv]] = A[:, [piv, k]]
                L[[k, piv], :k] = L[[piv, k], :k]
                perm[k], perm[piv] = perm[piv], perm[k]
                b[[k, piv]] = b[[piv, k]]
            D[k] = A[k, k]
            L[k, k] = 1.0
            L[k + 1:, k] = A[k + 1:, k] / D[k]
            for i in range(k + 1, n):
                for j in range(k + 1, n):
                    A[i, j] -= L[i, k] * D[k] * L[j, k]
        y = np.zeros(n)
        for i in range(n):
            y[i] = b[i] - sum(L[i, j] * y[j] for j in range(i))
        y /= D
        z = np.zeros(n)
        for i in range(n - 1, -1, -1):
            z[i] = y[i] - sum(L[j, i] * z[j] for j in range(i + 1, n))
    x = np.zeros(n)
    for i in range(n):
        x[perm[i]] = z[i]
    return x if np.all(np.isfinite(x)) else None


def delta_of(x):
    a, b, c = x[:3]
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    d = np.eye(4)
    d[:3, :3] = Rz @ Ry @ Rx
    d[:3, 3] = x[3:]
    return d


def optimize(src_xyz, tgt_xyz, corres, division_factor=1.4, use_absolute_scale=False, decrease_mu=False,
             maximum_correspondence_distance=0.025, iteration_number=64):
    """Normalisation, optimisation and the way back: dict(transformation (source -> target), n_corres, iterations, scale_global)."""
    P = np.asarray(src_xyz, np.float32).astype(np.float64)
    Q = np.asarray(tgt_xyz, np.float32).astype(np.float64)
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    mp, mq = fixed_order_mean(P), fixed_order_mean(Q)
    Pc, Qc = P - mp, Q - mq
    scale = max(np.sqrt((Pc[:, 0] * Pc[:, 0] + Pc[:, 1] * Pc[:, 1]) + Pc[:, 2] * Pc[:, 2]).max(),
                np.sqrt((Qc[:, 0] * Qc[:, 0] + Qc[:, 1] * Qc[:, 1]) + Qc[:, 2] * Qc[:, 2]).max())
    sg, mu = (1.0, scale) if use_absolute_scale else (scale, 1.0)
    with np.errstate(all="ignore"):               # a cloud of coincident points has scale 0: 0 / 0, as the library computes it
        Pc, Qc = Pc / sg, Qc / sg
    res = {"transformation": np.eye(4), "n_corres": len(corres), "iterations": 0, "scale_global": float(sg)}
    if len(corres) < 10:
        return res
    p, q = Pc[corres[:, 0]], Qc[corres[:, 1]].copy()
    trans = np.eye(4)
    for it in range(iteration_number):
        r = p - q
        with np.errstate(all="ignore"):
            l = (mu / ((r * r).sum(1) + mu)) ** 2
        z, o = np.zeros(len(q)), -np.ones(len(q))
        J = (np.stack([z, -q[:, 2], q[:, 1], o, z, z], 1), np.stack([q[:, 2], z, -q[:, 0], z, o, z], 1),
             np.stack([-q[:, 1], q[:, 0], z, z, z, o], 1))
        JTJ, JTr = np.zeros((6, 6)), np.zeros(6)
        for Jk, rk in zip(J, (r[:, 0], r[:, 1], r[:, 2])):
            JTJ += (Jk * l[:, None]).T @ Jk
            JTr += (Jk * (l * rk)[:, None]).sum(0)
        x = solve6_ldlt(-JTJ, JTr)
        if x is None:
            break
        d = delta_of(x)
        trans = d @ trans
        q = q @ d[:3, :3].T + d[:3, 3]
        if decrease_mu and it % 4 == 0 and mu > maximum_correspondence_distance:
            mu /= division_factor
        res["iterations"] = it + 1
    R, t = trans[:3, :3], trans[:3, 3]
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = -R @ mq + t * sg + mp
    res["transformation"] = np.linalg.inv(M)
    return res


def evaluate(src_xyz, tgt_xyz, max_corr, T, chunk=512):
    """Brute-force float64 EvaluateRegistration: (fitness, inlier_rmse, correspondence_set); inlier iff d2 < max_corr^2."""
    P = np.asarray(src_xyz, np.float32).astype(np.float64)
    Q = np.asarray(tgt_xyz, np.float32).astype(np.float64)
    moved = np.stack([T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1] + T[r, 2] * P[:, 2] + T[r, 3] for r in range(3)], 1)
    idx = np.empty(len(P), np.int64)
    d2 = np.empty(len(P))
    for s in range(0, len(P), chunk):
        d = moved[s:s + chunk, None, :] - Q[None]
        dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        idx[s:s + chunk] = dd.argmin(1)
        d2[s:s + chunk] = dd.min(1)
    inl = d2 < max_corr * max_corr
    good = int(inl.sum())
    rmse = math.sqrt(d2[inl].sum() / good) if good else 0.0
    return good / len(P), rmse, np.stack([np.flatnonzero(inl), idx[inl]], 1)


def fgr(src_xyz, tgt_xyz, corres, division_factor=1.4, use_absolute_scale=False, decrease_mu=False,
        maximum_correspondence_distance=0.025, iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, seed=0):
    """Steps 2-5 over the reciprocal pairs `corres`: the dict of optimize() plus n_reciprocal, n_trials, n_tuples."""
    used, n_trials = np.asarray(corres, np.int64), 0
    if tuple_test:
        used, n_trials = _tuple_test(src_xyz, tgt_xyz, corres, tuple_scale, maximum_tuple_count, seed)
    res = optimize(src_xyz, tgt_xyz, used, division_factor, use_absolute_scale, decrease_mu, maximum_correspondence_distance,
                   iteration_number)
    res.update(n_reciprocal=len(corres), n_trials=n_trials, n_tuples=len(used) // 3 if tuple_test else 0)
    return res
