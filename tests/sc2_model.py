"""Float64 NumPy model of the compatibility-graph global registration (test infrastructure, not the product).

The executable form of the definition in include/gsr_hip.h (gsr_sc2_correspondence).  ``sc2`` returns every
stage, and beside each float decision whether it is *decided*, i.e. far enough from its threshold that two correct float64
implementations must agree on it.
"""
from __future__ import annotations

import math

import numpy as np

import global_model as G

KMAX = 64
EMPTY = {"transformation": np.eye(4), "fitness": 0.0, "inlier_rmse": 0.0, "best_seed": -1, "best_index": -1, "n_seeds": 0, "n_valid": 0,
         "n_edges": 0, "refine_steps": 0, "host_waits": 0}


def lengths(X, rows=None):
    """a[i, j] = sqrt((dx * dx + dy * dy) + dz * dz) of X[rows[i]] - X[j], term by term as the kernel writes it."""
    A = X if rows is None else X[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        d = A[:, None, :] - X[None, :, :]
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def compatibility(P, Q, d_thr, chunk=512):
    """C (m, m) uint8: step 1."""
    m = len(P)
    C = np.zeros((m, m), np.uint8)
    for i0 in range(0, m, chunk):
        r = np.arange(i0, min(i0 + chunk, m))
        with np.errstate(invalid="ignore"):
            C[r] = np.abs(lengths(P, r) - lengths(Q, r)) < d_thr
    C[np.arange(m), np.arange(m)] = 0
    return C


def umeyama_sums(P, Q, members, ctr):
    """(T, sigma2 / sigma1) of step 5 / 7: the point-to-point sums about ctr and the estimator update of gsr_solve.h (rigid)."""
    p, q = P[members] - ctr, Q[members] - ctr
    n = float(len(members))
    mp, mq = p.sum(0) / n, q.sum(0) / n
    sigma = (q.T @ p) / n - np.outer(mq, mp)
    if not np.all(np.isfinite(sigma)):
        return np.full((4, 4), np.nan), 0.0
    U, s, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt.T) < 0:
        S[2] = -1.0
    R = (U * S) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq + ctr - R @ (mp + ctr)
    return T, (s[1] / s[0] if s[0] > 0 else 0.0)


def d2_of(T, P, Q):
    """d2 (m,) of every correspondence under T: the expression of k_ransac_eval, term by term."""
    with np.errstate(invalid="ignore", over="ignore"):
        X = [T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1] + T[r, 2] * P[:, 2] + T[r, 3] for r in range(3)]
        dx, dy, dz = X[0] - Q[:, 0], X[1] - Q[:, 1], X[2] - Q[:, 2]
        return dx * dx + dy * dy + dz * dz


def _score(T, P, Q, thr2):
    d2 = d2_of(T, P, Q)
    with np.errstate(invalid="ignore"):
        inl = d2 < thr2
        near = int((np.abs(d2 - thr2) < 1e-9 * thr2).sum())
    good = int(inl.sum())
    return good, (math.sqrt(d2[inl].sum() / good) if good else 0.0), near, inl


def _better(g, r, bg, br):
    return g > bg or (g == bg and r < br)


def _tie(g, r, bg, br):
    """True when (g, r) against (bg, br) is not decided: equal good and rmse within 1e-9 relative"""
    return g == bg and abs(r - br) <= 1e-9 * max(abs(r), abs(br))


def sc2(src_xyz, tgt_xyz, corres, d_thr, seed_ratio=0.2, max_seeds=4096, k1=30, k2=20, refine_iters=20):
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    m = len(corres)
    out = dict(EMPTY)
    if m < 3 or not (d_thr > 0):
        return out
    P = np.asarray(src_xyz, np.float32).astype(np.float64)[corres[:, 0]]
    Q = np.asarray(tgt_xyz, np.float32).astype(np.float64)[corres[:, 1]]
    thr2 = d_thr * d_thr
    # 1, 2
    C = compatibility(P, Q, d_thr)
    deg = C.sum(1, dtype=np.int64)
    n_seeds = int(min(max_seeds, math.ceil(seed_ratio * m), m))
    idx = np.arange(m)
    seeds = np.lexsort((idx, -deg))[:n_seeds]
    # 3: exact in float64 (the sums are integers <= m)
    Cf = C.astype(np.float64)
    rows = (C[seeds].astype(np.int64) * np.rint(Cf[seeds] @ Cf).astype(np.int64))
    # 4, 5
    K1 = np.full((n_seeds, KMAX), -1, np.int64)
    K2 = np.full((n_seeds, KMAX), -1, np.int64)
    hyp = np.tile(np.eye(4), (n_seeds, 1, 1))
    valid = np.zeros(n_seeds, bool)
    ratio = np.full(n_seeds, np.inf)
    for t, s in enumerate(seeds):
        cand = np.flatnonzero(C[s])
        a = np.concatenate([[s], cand[np.lexsort((cand, -rows[t, cand]))][: k1 - 1]])
        K1[t, : len(a)] = a
        l = C[np.ix_(a, a)].sum(1, dtype=np.int64)[1:]
        others = a[1:]
        b = np.concatenate([[s], others[np.lexsort((others, -l))][: k2 - 1]])
        K2[t, : len(b)] = b
        if len(b) < 3:
            continue
        mem = np.sort(b)
        try:
            T, ratio[t] = umeyama_sums(P, Q, mem, P[mem[0]])
        except np.linalg.LinAlgError:
            T = np.full((4, 4), np.nan)
        if np.all(np.isfinite(T)):
            hyp[t], valid[t] = T, True
    # 6
    good = np.full(n_seeds, -1, np.int64)
    rmse = np.zeros(n_seeds)
    near = np.zeros(n_seeds, np.int64)
    for t in np.flatnonzero(valid):
        good[t], rmse[t], near[t], _ = _score(hyp[t], P, Q, thr2)
    out.update(C=C, deg=deg, seeds=seeds, rows=rows, K1=K1, K2=K2, hyp=hyp, valid=valid, good=good, rmse=rmse, near=near, sigma_ratio=ratio,
               n_seeds=n_seeds, n_valid=int(valid.sum()), n_edges=int(deg.sum() // 2), host_waits=1,
               undecided_seeds=np.flatnonzero(valid & ((near > 0) | (ratio < 1e-3))))
    if not valid.any():
        out["decided"] = out["steps_decided"] = True
        return out
    v = np.flatnonzero(valid)
    order = v[np.lexsort((v, rmse[v], -good[v]))]
    best = int(order[0])
    decided = len(out["undecided_seeds"]) == 0
    # (a runner-up with the winner's very hypothesis -- the same K2 -- is no float decision: rank ascending settles it on both sides)
    if len(order) > 1 and _tie(good[order[1]], rmse[order[1]], good[best], rmse[best]) and not np.array_equal(hyp[order[1]], hyp[best]):
        decided = False
    steps_decided = True
    # 7
    T, g, r = hyp[best].copy(), int(good[best]), float(rmse[best])
    ctr = P[seeds[best]]
    steps, waits = 0, 1
    made_from = None                     # the inlier set T was estimated from (None: the seed's K2)
    for _ in range(refine_iters):
        inl = _score(T, P, Q, thr2)[3]
        waits += 1
        if inl.sum() < 3:
            break
        if made_from is not None and np.array_equal(inl, made_from):
            break                        # a fixed point: the same sums give the same T, good and rmse again, which is not better
        made_from = inl
        try:
            Tn, rt = umeyama_sums(P, Q, np.flatnonzero(inl), ctr)
        except np.linalg.LinAlgError:
            break
        if not np.all(np.isfinite(Tn)):
            break
        gn, rn, nn, _ = _score(Tn, P, Q, thr2)
        if nn or rt < 1e-3:
            decided = False
        elif _tie(gn, rn, g, r):
            # keep-or-stop is a coin flip.  Where the candidate IS the current transform up to rounding (the inliers are the set it was
            # made from, summed about another centre) only the step count depends on it, not the result
            steps_decided = False
            if np.abs(Tn - T).max() >= 1e-12:
                decided = False
        if not _better(gn, rn, g, r):
            break
        T, g, r = Tn, gn, rn
        steps += 1
    out.update(transformation=T, fitness=g / m, inlier_rmse=r, best_seed=best, best_index=int(seeds[best]), refine_steps=steps, host_waits=waits,
               decided=decided, steps_decided=steps_decided and decided)
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
D_THR = 0.05
T_PLANTED = G.make_T(120.0, (1.0, 2.0, 0.7), (0.3, -0.2, 0.5))


def planted(m, share, seed, sigma=0.01):
    """Planted correspondences: sources uniform in [-1, 1]^3 (float32); the first round(share * m) pairs (after a shuffle) are moved by
    T_PLANTED with sigma noise, the others are uniform in [-1.2, 1.2]^3.  The target rows are permuted, so corres is not the identity.
    -> (src float32, tgt float32, corres int32 (m, 2), inlier mask)"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    n_in = int(round(share * m))
    inl = np.zeros(m, bool)
    inl[rng.permutation(m)[:n_in]] = True
    moved = src.astype(np.float64) @ T_PLANTED[:3, :3].T + T_PLANTED[:3, 3] + sigma * rng.standard_normal((m, 3))
    tgt = np.where(inl[:, None], moved, rng.uniform(-1.2, 1.2, (m, 3))).astype(np.float32)
    perm = rng.permutation(m)
    tgt_rows = np.empty((m, 3), np.float32)
    tgt_rows[perm] = tgt
    corres = np.stack([np.arange(m), perm], 1).astype(np.int32)
    return src, tgt_rows, corres, inl


def pose_error(T, T_gt):
    return G.rotation_error_deg(T, T_gt), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))
