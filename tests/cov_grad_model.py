"""NumPy statement of the covariance build and its derivative (``csrc/gsr_covbuild.h``): the model ``k_cov_build`` and
``k_cov_build_backward`` are held to.

With a row's log-scales ``s`` and raw quaternion ``q = (w, x, y, z)``: ``n = |q|``, ``u = q / n``, ``e = exp(s)``, ``L = R(u) diag(e)``,
``cov = L L^T`` as ``(xx, xy, xz, yy, yz, zz)``.  With ``g6 = dLoss/dcov6`` in the convention of ``gsr_raster_backward`` (an off-diagonal
entry stands for both symmetric positions): ``G_ii = g6_ii``, ``G_ij = g6_ij / 2``, ``M = 2 G L``, ``dLoss/ds_k = e_k sum_i M_ik R_ik``,
``D_ik = M_ik e_k``, ``dLoss/du`` = ``D`` contracted with ``dR/du``, ``dLoss/dq = (dLoss/du - u (u . dLoss/du)) / n``.

``chain(s, q, g6, dtype)``: float64 by default; with ``dtype=np.float32`` every operation is a float32 operation in the kernel's order
(sums associated as ``(a + b) + c``).  A row whose six ``g6`` are all zero gets exact zeros in both gradients, as the contract says.

``chain(..., magnitude=True)`` is the error scale: the same expressions on the absolute values of the inputs with every subtraction
turned into an addition -- per output the sum of the absolute values of its terms, carried through the whole chain (so the scale of
``R_00 = 1 - 2 (y^2 + z^2)`` is ``1 + 2 (y^2 + z^2)`` also where the entry itself cancels to zero).  An error of an output is read against
it, the convention of ``tests/raster_grad_model.py``.
"""
from __future__ import annotations

import functools

import numpy as np

OUTPUTS = ("cov6", "scaling", "rotation")
SCENES = ("generic", "needles_discs", "special_rotations", "norms")
TINY = 1e-30


def chain(s, q, g6=None, dtype=np.float64, magnitude=False):
    """-> dict(cov6 (n,6); with g6 also scaling (n,3), rotation (n,4)) in ``dtype``"""
    f = np.dtype(dtype).type
    s = np.asarray(s, np.float32 if np.dtype(dtype) == np.float32 else np.float64).astype(dtype)
    q = np.asarray(q, s.dtype).astype(dtype)
    one, two, half = f(1), f(2), f(0.5)
    if magnitude:
        q = np.abs(q)
    sub = (lambda a, b: a + b) if magnitude else (lambda a, b: a - b)
    with np.errstate(all="ignore"):
        qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        nrm = np.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
        w, x, y, z = qw / nrm, qx / nrm, qy / nrm, qz / nrm
        e = [np.exp(s[:, k]) for k in range(3)]
        R = [[sub(one, two * (y * y + z * z)), two * sub(x * y, w * z), two * (x * z + w * y)],
             [two * (x * y + w * z), sub(one, two * (x * x + z * z)), two * sub(y * z, w * x)],
             [two * sub(x * z, w * y), two * (y * z + w * x), sub(one, two * (x * x + y * y))]]
        Lm = [[R[i][k] * e[k] for k in range(3)] for i in range(3)]
        cov = lambda i, j: (Lm[i][0] * Lm[j][0] + Lm[i][1] * Lm[j][1]) + Lm[i][2] * Lm[j][2]
        out = dict(cov6=np.stack([cov(0, 0), cov(0, 1), cov(0, 2), cov(1, 1), cov(1, 2), cov(2, 2)], 1))
        if g6 is None:
            return out
        g = np.asarray(g6, np.float32).astype(dtype)
        zero_row = ~g.any(axis=1)
        if magnitude:
            g = np.abs(g)
        G = [[g[:, 0], half * g[:, 1], half * g[:, 2]], [half * g[:, 1], g[:, 3], half * g[:, 4]], [half * g[:, 2], half * g[:, 4], g[:, 5]]]
        M = [[two * ((G[i][0] * Lm[0][k] + G[i][1] * Lm[1][k]) + G[i][2] * Lm[2][k]) for k in range(3)] for i in range(3)]
        gs = [e[k] * ((M[0][k] * R[0][k] + M[1][k] * R[1][k]) + M[2][k] * R[2][k]) for k in range(3)]
        D = [[M[i][k] * e[k] for k in range(3)] for i in range(3)]
        uw = two * ((x * sub(D[2][1], D[1][2]) + y * sub(D[0][2], D[2][0])) + z * sub(D[1][0], D[0][1]))
        ux = two * sub((y * (D[0][1] + D[1][0]) + z * (D[0][2] + D[2][0])) + w * sub(D[2][1], D[1][2]), (two * x) * (D[1][1] + D[2][2]))
        uy = two * sub((x * (D[0][1] + D[1][0]) + z * (D[1][2] + D[2][1])) + w * sub(D[0][2], D[2][0]), (two * y) * (D[0][0] + D[2][2]))
        uz = two * sub((x * (D[0][2] + D[2][0]) + y * (D[1][2] + D[2][1])) + w * sub(D[1][0], D[0][1]), (two * z) * (D[0][0] + D[1][1]))
        dot = ((w * uw + x * ux) + y * uy) + z * uz
        gq = [sub(uw, w * dot) / nrm, sub(ux, x * dot) / nrm, sub(uy, y * dot) / nrm, sub(uz, z * dot) / nrm]
        out["scaling"] = np.where(zero_row[:, None], f(0), np.stack(gs, 1))
        out["rotation"] = np.where(zero_row[:, None], f(0), np.stack(gq, 1))
    return out


def _directions(rng, n):
    d = rng.normal(size=(n, 4))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) + 3100


def make(name):
    """-> (scaling (n,3), rotation (n,4), grad_cov6 (n,6)) float32"""
    rng = np.random.default_rng(hash_name(name))
    if name == "generic":                       # s in [-6, 1], |q| in [0.1, 10]; the last eight rows have a zero gradient
        n = 300
        s = rng.uniform(-6.0, 1.0, (n, 3))
        q = _directions(rng, n) * 10.0 ** rng.uniform(-1.0, 1.0, (n, 1))
    elif name == "needles_discs":               # one axis 10 .. 10^4 times longer (needle) or shorter (disc) than the other two
        n = 200
        s = np.repeat(rng.uniform(-5.0, -3.0, (n, 1)), 3, 1) + rng.uniform(-0.1, 0.1, (n, 3))
        ratio = np.log(10.0 ** rng.uniform(1.0, 4.0, n))
        ratio[-2:] = np.log(1e4)
        axis = rng.integers(0, 3, n)
        s[np.arange(n), axis] += np.where(np.arange(n) % 2 == 0, ratio, -ratio)
        q = _directions(rng, n) * rng.uniform(0.5, 2.0, (n, 1))
    elif name == "special_rotations":           # identity, the three half-turns (w = 0), quaternions with one zero component; norms 1, 2.5, 0.3
        rows = [np.eye(4)[k] for k in range(4)]
        for k in range(4):
            d = _directions(rng, 12)
            d[:, k] = 0.0
            rows += list(d / np.linalg.norm(d, axis=1, keepdims=True))
        for a in ((1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 0), (0, 1, 1, 1), (1, -1, 0, 0)):      # quarter and third turns
            rows.append(np.float64(a))
        q = np.concatenate([np.stack(rows) * c for c in (1.0, 2.5, 0.3)])
        n = len(q)
        s = rng.uniform(-4.0, 0.0, (n, 3))
    elif name == "norms":                       # |q| = 1e-3 and 1e3: the gradient of the quaternion scales with 1 / |q|
        n = 200
        s = rng.uniform(-4.0, 0.0, (n, 3))
        q = _directions(rng, n) * np.where(np.arange(n) % 2 == 0, 1e-3, 1e3)[:, None]
    else:
        raise KeyError(name)
    g = rng.normal(size=(n, 6))
    if name == "generic":
        g[-8:] = 0.0
    return s.astype(np.float32), q.astype(np.float32), g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_models(name):
    """Everything the tests need of a scene, computed once and left unchanged: the inputs, the float64 model and its scale"""
    s, q, g = make(name)
    ref = chain(s, q, g)
    scale = chain(s, q, g, magnitude=True)
    for a in (s, q, g) + tuple(ref[k] for k in OUTPUTS) + tuple(scale[k] for k in OUTPUTS):
        a.setflags(write=False)
    return dict(scaling=s, rotation=q, grad_cov6=g, ref=ref, scale=scale)


def error(name, got, output):
    """max |got - float64 model| / (scale + TINY) over the rows of a scene, for one output"""
    m = scene_models(name)
    return float((np.abs(np.asarray(got, np.float64) - m["ref"][output]) / (m["scale"][output] + TINY)).max())


def float32_cost(name):
    """what float32 costs the model itself, per output"""
    m = scene_models(name)
    g32 = chain(m["scaling"], m["rotation"], m["grad_cov6"], np.float32)
    assert all(g32[k].dtype == np.float32 for k in OUTPUTS)
    return {k: error(name, g32[k], k) for k in OUTPUTS}
