"""Similarities ``[c R | t]`` -- what a registration with scaling returns -- in plain NumPy (no kernel).

* ``split_similarity(T) -> (c, R, t)`` with the gate of ``gsr_model_similarity`` (``include/gsr_hip.h``): ``det A > 0``,
  ``c = cbrt(det A)`` in ``[1e-6, 1e6]``, ``max|A^T A / c^2 - I| <= 1e-3``; anything else is a ``ValueError``.
* ``initial_similarity(source_xyz, target_xyz) -> 4x4``: centroids aligned, ``c`` = RMS radius of the target / RMS radius of the
  source, no rotation -- a start for ICP with scaling when no global method ran (two scenes from separate structure-from-motion runs
  differ by an arbitrary factor, and ICP's correspondence distance means nothing until the sizes roughly agree).
"""
from __future__ import annotations

import numpy as np

GATE = 1e-3
C_MIN, C_MAX = 1e-6, 1e6


def _host(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def split_similarity(T):
    """-> ``(c, R, t)``: float, (3, 3) and (3,) float64 with ``T[:3, :3] = c R``."""
    T = _host(T)
    if T.shape != (4, 4):
        raise ValueError(f"split_similarity: a 4x4 matrix is needed, got {T.shape}")
    A, t = T[:3, :3], T[:3, 3].copy()
    det = float(np.linalg.det(A))
    if not det > 0.0:
        raise ValueError("split_similarity: the upper 3x3 is not c R with c > 0 (det <= 0: a reflection or a singular matrix)")
    c = float(np.cbrt(det))
    if not (C_MIN <= c <= C_MAX):
        raise ValueError(f"split_similarity: scale {c:g} outside [{C_MIN:g}, {C_MAX:g}]")
    R = A / c
    worst = float(np.abs(R.T @ R - np.eye(3)).max())
    if not worst <= GATE:
        raise ValueError(f"split_similarity: the upper 3x3 is not c R (max|A^T A / c^2 - I| = {worst:.3g} > {GATE:g})")
    return c, R, t


def rms_radius(xyz):
    """Root mean square distance of the points from their centroid (float64)."""
    p = _host(xyz).reshape(-1, 3)
    if len(p) == 0:
        return 0.0
    d = p - p.mean(0)
    return float(np.sqrt((d * d).sum(1).mean()))


def initial_similarity(source_xyz, target_xyz):
    """4x4 ``[c I | mt - c ms]``: the source's centroid ``ms`` lands on the target's ``mt``, its RMS radius becomes the target's."""
    p, q = _host(source_xyz).reshape(-1, 3), _host(target_xyz).reshape(-1, 3)
    if len(p) == 0 or len(q) == 0:
        raise ValueError("initial_similarity: empty cloud")
    rs, rt = rms_radius(p), rms_radius(q)
    if not (rs > 0.0 and rt > 0.0):
        raise ValueError("initial_similarity: a cloud of coincident points has no size")
    c = rt / rs
    T = np.eye(4)
    T[:3, :3] *= c
    T[:3, 3] = q.mean(0) - c * p.mean(0)
    return T
