"""The float64 model of the colour harmonisation, independent of the library's route:

  * the sums of an edge by ``math.fsum`` over the pairs (exactly rounded sums of float64 terms);
  * the fit NOT from the sums: least squares on the stacked, weighted design built from the raw pairs, the prior as extra rows --
    ``numpy.linalg.lstsq`` (``route="lstsq"``), a Householder QR in ``longdouble`` (``"qr_longdouble"``, the most accurate route and
    the one the library is compared with) or the float64 normal equations of that design (``"normal"``).  The distance between the
    last two on an input is that input's delta: what two honest float64 routes differ by;
  * the transform applied to a model in float64.
"""
import math

import numpy as np

C0 = 0.28209479177387814
SUMS_LEN = 40
MODES = {"gain": 1, "channel_gain": 3, "affine": 12}
I0 = np.hstack([np.eye(3), np.zeros((3, 1))])


def base(dc):
    return 0.5 + C0 * np.asarray(dc, np.float32).astype(np.float64)


def sigmoid(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(o, np.float32).astype(np.float64)))


def pair_terms(s_dc, s_op, t_dc, t_op, pairs, Ps=I0, Pt=I0, k=math.inf):
    """-> dict: a, b (m, 4), w, rho2 (m,) of the pairs that count, and the two counts"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    ns, nt = len(s_dc), len(t_dc)
    inside = (pairs[:, 0] >= 0) & (pairs[:, 0] < ns) & (pairs[:, 1] >= 0) & (pairs[:, 1] < nt)
    pin = pairs[inside]
    s_dc, t_dc = np.asarray(s_dc, np.float32).reshape(ns, 3), np.asarray(t_dc, np.float32).reshape(nt, 3)
    s_op, t_op = np.asarray(s_op, np.float32).reshape(ns), np.asarray(t_op, np.float32).reshape(nt)
    fin = (np.isfinite(s_dc[pin[:, 0]]).all(1) & np.isfinite(s_op[pin[:, 0]]) & np.isfinite(t_dc[pin[:, 1]]).all(1) & np.isfinite(t_op[pin[:, 1]]))
    i, j = pin[fin, 0], pin[fin, 1]
    a = np.hstack([base(s_dc[i]), np.ones((len(i), 1))])
    b = np.hstack([base(t_dc[j]), np.ones((len(j), 1))])
    u = sigmoid(s_op[i]) * sigmoid(t_op[j])
    r = a @ np.asarray(Ps, np.float64).reshape(3, 4).T - b @ np.asarray(Pt, np.float64).reshape(3, 4).T
    rho2 = (r * r).sum(1)
    rho = np.sqrt(rho2)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(rho > k, k / rho, 1.0)
    return {"a": a, "b": b, "w": u * h, "rho2": rho2, "i": i, "j": j, "n_skipped": int((~fin).sum()), "n_out_of_range": int((~inside).sum())}


def sums(s_dc, s_op, t_dc, t_op, pairs, Ps=I0, Pt=I0, k=math.inf):
    """-> (sums (40,), abs_sums (40,), n_skipped, n_out_of_range): every sum by fsum; abs_sums = fsum of the terms' magnitudes"""
    T = pair_terms(s_dc, s_op, t_dc, t_op, pairs, Ps, Pt, k)
    a, b, w = T["a"], T["b"], T["w"]
    cols = [np.ones(len(w)), w, w * T["rho2"]]
    cols += [w * a[:, r] * a[:, c] for r in range(4) for c in range(r, 4)]
    cols += [w * a[:, r] * b[:, c] for r in range(4) for c in range(4)]
    cols += [w * b[:, r] * b[:, c] for r in range(4) for c in range(r, 4)]
    S = np.array([math.fsum(c) for c in cols] + [0.0])
    A = np.array([math.fsum(np.abs(c)) for c in cols] + [0.0])
    return S, A, T["n_skipped"], T["n_out_of_range"]


def basis(mode):
    d = MODES[mode]
    B = np.zeros((d, 3, 4))
    if mode == "gain":
        B[0, :, :3] = np.eye(3)
    elif mode == "channel_gain":
        for c in range(3):
            B[c, c, c] = 1.0
    else:
        B = np.eye(12).reshape(12, 3, 4)
    return B


def held_nodes(N, edges, counts, min_pairs, reference):
    seen = {reference}
    grew = True
    while grew:
        grew = False
        for (s, t), n in zip(edges, counts):
            if n >= min_pairs and ((s in seen) != (t in seen)):
                seen |= {s, t}
                grew = True
    return np.array([i not in seen or i == reference for i in range(N)])


def lstsq_qr(A, y, dtype=np.longdouble):
    """least squares by Householder QR in ``dtype`` (numpy's LAPACK routes stop at float64)"""
    A, y = np.array(A, dtype=dtype), np.array(y, dtype=dtype)
    m, n = A.shape
    for k in range(n):
        x = A[k:, k]
        alpha = -np.copysign(np.sqrt((x * x).sum()), x[0])
        v = x.copy()
        v[0] -= alpha
        vv = (v * v).sum()
        if vv == 0:
            continue
        A[k:, k:] -= np.outer(v, (2 / vv) * (v @ A[k:, k:]))
        y[k:] -= v * ((2 / vv) * (v @ y[k:]))
    x = np.zeros(n, dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - A[k, k + 1:n] @ x[k + 1:]) / A[k, k]
    return x.astype(np.float64)


def fit(P, edges, terms, mode, prior, min_pairs, reference, route="qr_longdouble"):
    """One weighted least-squares solve from the raw pairs.  P (N, 3, 4): held nodes keep theirs; edges: [(s, t)]; terms: per edge
    the dict of pair_terms (a, b, w at the current transforms) -> (P_new, held)"""
    P = np.array(P, np.float64).reshape(-1, 3, 4)
    N, B, d = len(P), basis(mode), MODES[mode]
    held = held_nodes(N, edges, [len(T["w"]) for T in terms], min_pairs, reference)
    var = {}
    for i in range(N):
        if not held[i]:
            var[i] = d * len(var)
    n_unk = d * len(var)
    if n_unk == 0:
        return P, held
    lam = prior * math.fsum(math.fsum(T["w"]) for T in terms) / len(edges) if edges else 0.0
    rows, rhs = [], []
    for (s, t), T in zip(edges, terms):
        q = np.sqrt(T["w"])
        for c in range(3):
            R = np.zeros((len(q), n_unk))
            y = np.zeros(len(q))
            if s in var:
                for k in range(d):
                    R[:, var[s] + k] += q * (T["a"] @ B[k, c])
            else:
                y -= q * (T["a"] @ P[s, c])
            if t in var:
                for k in range(d):
                    R[:, var[t] + k] -= q * (T["b"] @ B[k, c])
            else:
                y += q * (T["b"] @ P[t, c])
            rows.append(R)
            rhs.append(y)
    for i, v in var.items():
        R = np.zeros((12, n_unk))
        for k in range(d):
            R[:, v + k] = math.sqrt(lam) * B[k].reshape(12)
        rows.append(R)
        rhs.append(math.sqrt(lam) * I0.reshape(12))
    A, y = np.vstack(rows), np.concatenate(rhs)
    if route == "lstsq":
        theta = np.linalg.lstsq(A, y, rcond=None)[0]
    elif route == "qr_longdouble":
        theta = lstsq_qr(A, y)
    elif route == "normal":
        theta = np.linalg.solve(A.T @ A, A.T @ y)
    else:
        raise ValueError(route)
    out = P.copy()
    for i, v in var.items():
        out[i] = np.tensordot(theta[v:v + d], B, axes=1)
    return out, held


def irls(cols, edges, pair_lists, mode="affine", huber=0.1, iterations=5, prior=1e-4, min_pairs=100, reference=0, route="qr_longdouble", P0=None):
    """The robust fit: cols[i] = (dc (n, 3), opacity (n,)) of scene i; start at P0 (identity); `iterations` times: the weights of every
    edge at the current transforms, then the solve -> (P (N, 3, 4), held)"""
    N = len(cols)
    P = np.tile(I0, (N, 1, 1)) if P0 is None else np.array(P0, np.float64).reshape(N, 3, 4)
    held = np.ones(N, bool)
    for _ in range(iterations):
        terms = [pair_terms(cols[s][0], cols[s][1], cols[t][0], cols[t][1], pl, P[s], P[t], huber) for (s, t), pl in zip(edges, pair_lists)]
        P, held = fit(P, edges, terms, mode, prior, min_pairs, reference, route)
    return P, held


def delta(*args, **kw):
    """what the float64 normal equations and the longdouble QR differ by on this input: the largest coefficient difference"""
    Pn, _ = irls(*args, route="normal", **kw)
    Pq, _ = irls(*args, route="qr_longdouble", **kw)
    return float(np.abs(Pn - Pq).max()), Pq


def apply(P, dc, sh=None):
    """-> (dc', sh') in float64: dc' = M dc + (M 0.5 + b - 0.5) / C0, sh'_k = M sh_k; dc (n, 3), sh (n, K, 3)"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    M, b = P[:, :3], P[:, 3]
    dc = np.asarray(dc, np.float32).astype(np.float64).reshape(-1, 3)
    off = (M @ np.full(3, 0.5) + b - 0.5) / C0
    out_dc = dc @ M.T + off
    out_sh = None
    if sh is not None:
        out_sh = np.asarray(sh, np.float32).astype(np.float64) @ M.T
    return out_dc, out_sh


def distort(P, dc):
    """the float32 dc whose base colour is P applied to the base colour of `dc` (how a test makes a scene with another exposure)"""
    return apply(P, dc)[0].astype(np.float32)
