"""Mixture-to-mixture registration: a Gaussian mixture set against a Gaussian mixture.  Every source component
interacts with every target component within ``max_corr``, weighted by ``w_i v_j exp(-m / 2)`` with ``m`` the Mahalanobis distance
under ``cov_scale^2 (R A_i R' + B_j) + cov_floor I`` -- no nearest neighbour, no correspondence that could flip between iterations.
The reference has no such method.  The definition is the header comment of ``include/gsr_hip.h``; ``tests/d2d_model.py`` restates it
in float64 NumPy.

``D2DContext`` (``gsr_d2d_*``: the target's grid, covariances and weights, the source; ``accumulate`` -> the 32 sums, ``register`` ->
the IRLS loop) and ``register_levels`` (coarse to fine over mixture levels).  Rigid only; one device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as _m

SUMS_LEN = _lib.GSR_D2D_SUMS_LEN
SLOT_SCORE, SLOT_WM, SLOT_PAIRS, SLOT_ROWS, SLOT_SINGULAR = 27, 28, 29, 30, 31


def unpack_sums(sums):
    """-> ``(H (6, 6), g (6,))`` of the 32 sums: rotation rows first, the increment acts on the left"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[:21]
    return H + np.triu(H, 1).T, np.array(sums[21:27])


class D2DContext:
    """``with D2DContext(device) as ctx: ctx.set_target(xyz, cov6, weight, max_corr); ctx.set_source(xyz, cov6, weight)``.
    Arrays are numpy (staged by the library) or CUDA tensors of this device (read in place); ``weight`` may be ``None`` (all 1).
    A communicator is not supported: a context used with one is refused."""

    def __init__(self, device=0, stream=None, comm=None):
        if comm is not None:
            raise RuntimeError("mixture-to-mixture registration has no multi-GPU split: a D2DContext cannot be used with a communicator")
        self._L = _lib.load(require_device=True)
        self.device = int(device)
        try:
            import torch
            if stream is None and torch.cuda.is_available():
                stream = torch.cuda.current_stream(self.device).cuda_stream
        except ImportError:  # pragma: no cover
            pass
        h = C.c_void_p()
        _lib.check(self._L.gsr_d2d_create(C.byref(h), self.device, C.c_void_p(stream or 0)), "gsr_d2d_create")
        self._h = h
        self.n_source = self.n_target = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsr_d2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _arrays(self, xyz, cov6, weight):
        n = int(xyz.shape[0])
        px, kx, dx = _m.prep(xyz, (n, 3), np.float32, self.device)
        pc, kc, dc = _m.prep(cov6, (n, 6), np.float32, self.device)
        pw, kw, dw = _m.prep(weight, (n,), np.float32, self.device)
        if dc != dx or (weight is not None and dw != dx):
            raise RuntimeError("centres, covariances and weights must live in the same place (all host or all device)")
        if dx:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        return n, px if n else None, pc if n else None, pw if n else None, 1 if dx else 0, (kx, kc, kw)

    def set_target(self, xyz, cov6, weight, max_corr):
        n, px, pc, pw, on, keep = self._arrays(xyz, cov6, weight)
        _lib.check(self._L.gsr_d2d_set_target(self._h, px, pc, pw, n, float(max_corr), on), "gsr_d2d_set_target")
        self.n_target = n

    def set_source(self, xyz, cov6, weight=None):
        n, px, pc, pw, on, keep = self._arrays(xyz, cov6, weight)
        _lib.check(self._L.gsr_d2d_set_source(self._h, px, pc, pw, n, on), "gsr_d2d_set_source")
        self.n_source = n

    def accumulate(self, T, cov_scale=1.0, cov_floor=0.0):
        """-> the 32 float64 sums at ``T`` (``gsr_d2d_accumulate``): H's upper triangle, g, the score, sum omega m and the counts"""
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4))
        out = np.empty(SUMS_LEN, np.float64)
        _lib.check(self._L.gsr_d2d_accumulate(self._h, T.ctypes.data, float(cov_scale), float(cov_floor), out.ctypes.data), "gsr_d2d_accumulate")
        return out

    def register(self, init, cov_scale=1.0, cov_floor=0.0, relative_score=1e-6, max_iteration=30):
        """-> dict: ``transformation`` (4, 4), ``score``, ``fitness``, ``mahalanobis_rmse``, ``iterations``, ``status``, ``n_pairs``,
        ``n_singular`` (``gsr_d2d_register``)"""
        T0 = np.ascontiguousarray(np.asarray(init, dtype=np.float64).reshape(4, 4))
        T = np.empty((4, 4), np.float64)
        R = _lib.D2DReport()
        _lib.check(self._L.gsr_d2d_register(self._h, T0.ctypes.data, float(cov_scale), float(cov_floor), float(relative_score), int(max_iteration),
                                            T.ctypes.data, C.addressof(R)), "gsr_d2d_register")
        return dict(transformation=T, score=float(R.score), fitness=float(R.fitness), mahalanobis_rmse=float(R.mahalanobis_rmse),
                    iterations=int(R.iterations), status=_lib.GSR_D2D_STATUS[int(R.status)], n_pairs=int(R.n_pairs), n_singular=int(R.n_singular))


def level_arrays(level):
    """-> ``(xyz, cov6, weight or None)`` of a mixture level: a ``PointCloud`` record (``xyz32``, ``cov6``; a ``weight`` attribute when
    it has one) or a level dict of ``hem.create_mixture`` (``"xyz"``, ``"cov6"``, ``"weight"`` when it carries it)"""
    if isinstance(level, dict):
        return level["xyz"], level["cov6"], level.get("weight")
    if getattr(level, "cov6", None) is None:
        raise RuntimeError("mixture-to-mixture registration needs covariances on both clouds")
    return level.xyz32, level.cov6, getattr(level, "weight", None)


def _device_of(level, device):
    if device is not None:
        return int(device)
    xyz = level_arrays(level)[0]
    return xyz.device.index if _m.is_cuda(xyz) else int(getattr(level, "device_index", 0))


def register_pair(source, target, init, max_corr, cov_scale=1.0, cov_floor=0.0, relative_score=1e-6, max_iteration=30, source_weights=None,
                  target_weights=None, device=None, ctx=None):
    """one registration of two levels (see ``level_arrays``); explicit weights override the levels' own"""
    sx, sc, sw = level_arrays(source)
    tx, tc, tw = level_arrays(target)
    sw = sw if source_weights is None else source_weights
    tw = tw if target_weights is None else target_weights
    own = ctx is None
    if own:
        ctx = D2DContext(_device_of(target, device))
    try:
        ctx.set_target(tx, tc, tw, max_corr)
        ctx.set_source(sx, sc, sw)
        return ctx.register(init, cov_scale, cov_floor, relative_score, max_iteration)
    finally:
        if own:
            ctx.close()


def register_levels(source_levels, target_levels, init, max_corr_values, cov_scale_values, iter_values, cov_floor=0.0, relative_score=1e-6, device=None):
    """Coarse to fine: entry ``k`` registers ``source_levels[-(k + 1)]`` against ``target_levels[-(k + 1)]`` (the last list entry is the
    coarsest level, as in the multiscale ICP worker) with ``max_corr_values[k]``, ``cov_scale_values[k]`` and at most ``iter_values[k]``
    steps, starting from the previous entry's transform.  -> ``(last result dict, [every entry's result])``"""
    n = len(iter_values)
    if len(source_levels) != len(target_levels):
        raise ValueError("the two lists of mixture levels differ in size")
    if not (len(max_corr_values) == len(cov_scale_values) == n) or n == 0 or n > len(source_levels):
        raise ValueError("max_corr, cov_scale and iteration values must have one entry per level used")
    T = np.asarray(init, dtype=np.float64).reshape(4, 4)
    results = []
    with D2DContext(_device_of(target_levels[0], device)) as ctx:
        for k in range(n):
            r = register_pair(source_levels[-(k + 1)], target_levels[-(k + 1)], T, max_corr_values[k], cov_scale_values[k], cov_floor, relative_score,
                              iter_values[k], ctx=ctx)
            results.append(r)
            T = r["transformation"]
    return results[-1], results
