"""Non-rigid refinement: a trilinear lattice of node displacements that absorbs the smooth, low-frequency
drift a single matrix leaves between two scenes.  The reference has no such step.

``WarpLattice`` (box + nodes per axis), ``WarpField`` (lattice + displacements ``U``; ``apply_points``, ``apply_arrays``, ``save`` /
``load``), ``WarpContext`` (``gsr_warp_*``: the target's grid and normals, the source, ``accumulate``), ``solve``
(``gsr_warp_solve``: host code, works without a GPU) and ``NonRigidRefiner`` (the coarse-to-fine loop).  The definitions are those of
``include/gsr_hip.h``; ``tests/warp_model.py`` restates them in float64 NumPy.

Only the source moves.  The field lives in the COMMON frame: the source is moved by ``init`` (rigid or a similarity) first, and a
point's cell and weights always come from that position, never from the warped one.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field as _dc_field

import numpy as np

from . import _lib
from . import _marshal as _m
from . import _model_view as _mv

CELL_LEN = _lib.GSR_WARP_CELL_LEN
MIN_DIM, MAX_DIM = 2, 17


def default_box(points):
    """-> (lo, hi) float64: the bounding box of the finite rows of ``points``, every axis widened symmetrically to at least 1e-3 of
    the largest extent, then padded by 1e-6 of the largest extent on every side."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if p.shape[0] == 0:
        raise ValueError("no finite point to put a lattice around")
    lo, hi = p.min(axis=0), p.max(axis=0)
    big = float((hi - lo).max())
    if not big > 0:
        big = 1.0                                   # a single point: a unit box around it
    short = np.maximum(1e-3 * big - (hi - lo), 0.0) * 0.5
    lo, hi = lo - short, hi + short
    return lo - 1e-6 * big, hi + 1e-6 * big


class WarpLattice:
    """``dims = (nx, ny, nz)`` nodes per axis (2 .. 17 each) over the box ``lo .. hi``; node ``(ix, iy, iz)`` has index
    ``(ix ny + iy) nz + iz``, spacing ``h_a = (hi_a - lo_a) / (n_a - 1)``."""

    def __init__(self, lo, hi, dims):
        self.lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float64).reshape(3))
        self.hi = np.ascontiguousarray(np.asarray(hi, dtype=np.float64).reshape(3))
        self.dims = np.ascontiguousarray(np.asarray(dims, dtype=np.int32).reshape(3))
        if (self.dims < MIN_DIM).any() or (self.dims > MAX_DIM).any():
            raise ValueError(f"lattice dimensions {tuple(int(d) for d in self.dims)} outside [{MIN_DIM}, {MAX_DIM}]")
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.hi > self.lo).all()):
            raise ValueError(f"lattice box {self.lo} .. {self.hi} is not a box")

    @property
    def h(self):
        return (self.hi - self.lo) / (self.dims - 1).astype(np.float64)

    @property
    def n_nodes(self):
        return int(np.prod(self.dims))

    @property
    def n_cells(self):
        return int(np.prod(self.dims - 1))

    def node_positions(self):
        """-> (M, 3) float64, in node order"""
        ax = [self.lo[a] + np.arange(self.dims[a], dtype=np.float64) * self.h[a] for a in range(3)]
        g = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)
        return g.reshape(-1, 3)

    def with_dims(self, dims):
        return WarpLattice(self.lo, self.hi, dims)

    def _args(self):
        return self.lo.ctypes.data, self.hi.ctypes.data, self.dims.ctypes.data


def _is_cuda(a):
    return _m.is_cuda(a)


class WarpField:
    """A lattice and its node displacements ``U`` (M, 3) float64: ``d(p) = sum_k w_k U_k`` over the eight nodes of ``p``'s cell."""

    def __init__(self, lattice, U=None):
        self.lattice = lattice
        M = lattice.n_nodes
        self.U = np.zeros((M, 3), np.float64) if U is None else np.ascontiguousarray(np.asarray(U, dtype=np.float64).reshape(M, 3))

    def is_identity(self):
        return not self.U.any()

    def displacement(self, points):
        """``d(p)`` of float64 points on the host (NumPy): what the prolongation evaluates at the finer lattice's nodes.  Not a hot
        path: the kernels (``apply_points``, ``apply_arrays``) move clouds and models."""
        L = self.lattice
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        n, h = L.dims.astype(np.int64), L.h
        sb = np.minimum(np.maximum((p - L.lo) / h, 0.0), (n - 1).astype(np.float64))
        c = np.minimum(np.floor(sb).astype(np.int64), n - 2)
        f = sb - c
        d = np.zeros_like(p)
        for k in range(8):
            b = np.array([(k >> 2) & 1, (k >> 1) & 1, k & 1])
            w = np.where(b == 1, f, 1.0 - f)
            node = ((c[:, 0] + b[0]) * n[1] + c[:, 1] + b[1]) * n[2] + c[:, 2] + b[2]
            d += ((w[:, 0] * w[:, 1]) * w[:, 2])[:, None] * self.U[node]
        return d

    def prolong(self, dims):
        """-> the same field on a lattice of ``dims`` nodes over the same box: the coarser field evaluated at the finer nodes.  Exact
        when every coarse node is a fine node (2^l + 1 -> 2^(l+1) + 1)."""
        fine = self.lattice.with_dims(dims)
        return WarpField(fine, self.displacement(fine.node_positions()))

    def apply_points(self, xyz, device=None):
        """-> ``float32(p + d(p))`` (``gsr_warp_points``): a CUDA tensor for a CUDA tensor, else a numpy array.  Rows with a non-finite
        coordinate come back unchanged; ``U == 0`` gives the input's bits."""
        L = _lib.load(require_device=True)
        n = int(xyz.shape[0])
        if device is None:
            device = xyz.device.index if _is_cuda(xyz) else 0
        p, keep, on = _m.prep(xyz, (n, 3), np.float32, device)
        out, pout = _m.out((n, 3), np.float32, device, on)
        _lib.check(L.gsr_warp_points(*self.lattice._args(), self.U.ctypes.data, p, n, pout, *_mv.call_tail(device, on)), "gsr_warp_points")
        return out

    def apply_arrays(self, xyz, cov6, device=None):
        """-> ``(xyz', cov6', n_folded)`` (``gsr_model_warp``): positions ``float32(p + d(p))``, covariances ``F cov F'`` with
        ``F = I + sum_k U_k grad w_k'``; ``n_folded`` counts the rows with ``det F <= 0``."""
        L = _lib.load(require_device=True)
        n = int(xyz.shape[0])
        if device is None:
            device = xyz.device.index if _is_cuda(xyz) else 0
        px, kx, on = _m.prep(xyz, (n, 3), np.float32, device)
        pc, kc, on_c = _m.prep(cov6, (n, 6), np.float32, device)
        if on_c != on:
            raise RuntimeError("positions and covariances must live in the same place (both host or both device)")
        ox, pox = _m.out((n, 3), np.float32, device, on)
        oc, poc = _m.out((n, 6), np.float32, device, on)
        folded = C.c_int64(0)
        _lib.check(L.gsr_model_warp(*self.lattice._args(), self.U.ctypes.data, n, px, pc, pox, poc, C.byref(folded), *_mv.call_tail(device, on)),
                   "gsr_model_warp")
        return ox, oc, int(folded.value)

    def save(self, path):
        """the field as ``.npz``: ``lo``, ``hi``, ``dims``, ``U``"""
        with open(path, "wb") as f:
            np.savez(f, lo=self.lattice.lo, hi=self.lattice.hi, dims=self.lattice.dims, U=self.U)

    @staticmethod
    def load(path):
        with np.load(path) as z:
            return WarpField(WarpLattice(z["lo"], z["hi"], z["dims"]), z["U"])


def solve(dims, sums, lam, lam0, U=None):
    """``gsr_warp_solve`` -> ``(U, report)``: the minimiser of the energy at the correspondences behind ``sums``
    ((ncells, 326) float64) and the report (``E_before`` at the ``U`` handed in, ``E_after``, the data terms, ``n_corr``,
    ``n_unknowns``, ``half_band``, ``pivot_min`` / ``pivot_max``).  Host code: works without a GPU.  A refusal is a ``RuntimeError``."""
    L = _lib.load()
    d = np.ascontiguousarray(np.asarray(dims, dtype=np.int32).reshape(3))
    ok = bool((d >= MIN_DIM).all() and (d <= MAX_DIM).all())
    M = int(np.prod(d.astype(np.int64))) if ok else 1
    ncells = int(np.prod(d.astype(np.int64) - 1)) if ok else 1
    s = np.ascontiguousarray(np.asarray(sums, dtype=np.float64).reshape(ncells, CELL_LEN) if ok else np.zeros((1, CELL_LEN)))
    u = np.zeros((M, 3), np.float64) if U is None else np.array(np.asarray(U, dtype=np.float64).reshape(M, 3), order="C", copy=True)
    R = _lib.WarpReport()
    _lib.check(L.gsr_warp_solve(d.ctypes.data, s.ctypes.data, float(lam), float(lam0), u.ctypes.data, C.addressof(R)), "gsr_warp_solve")
    return u, {k: (float if isinstance(getattr(R, k), float) else int)(getattr(R, k)) for k, _ in R._fields_}


class WarpContext:
    """The target's point grid with its normals, built once, and the source points (``gsr_warp_create`` ...)."""

    def __init__(self, device=0, stream=None):
        self._L = _lib.load(require_device=True)
        self.device = int(device)
        try:
            import torch
            if stream is None and torch.cuda.is_available():
                stream = torch.cuda.current_stream(self.device).cuda_stream
        except ImportError:  # pragma: no cover
            pass
        h = C.c_void_p()
        _lib.check(self._L.gsr_warp_create(C.byref(h), self.device, C.c_void_p(stream or 0)), "gsr_warp_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsr_warp_destroy(self._h)
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

    def _sync_torch(self):
        import torch
        torch.cuda.current_stream(self.device).synchronize()

    def set_target(self, xyz, normals, max_corr):
        n = int(xyz.shape[0])
        px, kx, dx = _m.prep(xyz, (n, 3), np.float32, self.device)
        pn, kn, dn = _m.prep(normals, (n, 3), np.float64, self.device)
        if dn != dx:
            raise RuntimeError("target points and normals must live in the same place (both host or both device)")
        if dx:
            self._sync_torch()
        _lib.check(self._L.gsr_warp_set_target(self._h, px, pn, n, float(max_corr), 1 if dx else 0), "gsr_warp_set_target")

    def set_source(self, xyz):
        n = int(xyz.shape[0])
        px, kx, dx = _m.prep(xyz, (n, 3), np.float32, self.device)
        if dx:
            self._sync_torch()
        _lib.check(self._L.gsr_warp_set_source(self._h, px if n else None, n, 1 if dx else 0), "gsr_warp_set_source")

    def accumulate(self, field):
        """-> ``(sums (ncells, 326) float64, n_corr, rmse)`` at the correspondences of the source warped by ``field``"""
        sums = np.empty((field.lattice.n_cells, CELL_LEN), np.float64)
        n, rmse = C.c_int64(0), C.c_double(0.0)
        _lib.check(self._L.gsr_warp_accumulate(self._h, *field.lattice._args(), field.U.ctypes.data, sums.ctypes.data, C.byref(n), C.byref(rmse)),
                   "gsr_warp_accumulate")
        return sums, int(n.value), float(rmse.value)


@dataclass
class WarpResult:
    field: WarpField = None
    levels: list = _dc_field(default_factory=list)      # per level: {"dims", "iterations": [{"n_corr", "rmse", "E_before", "E_after"}]}
    n_corr: int = 0                                     # at the final field
    rmse_before: float = 0.0                            # point-to-plane RMSE of the correspondences without the warp
    rmse_after: float = 0.0                             # and of those at the final field
    n_folded: int = 0                                   # source points where det F <= 0
    timings: dict = _dc_field(default_factory=dict)     # seconds: "build", "accumulate", "solve", "total"


def _moved_f32(xyz, T):
    """the source in the common frame: ``float32(A p + t)`` computed in float64; placement kept"""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    if np.array_equal(T, np.eye(4)):
        return xyz
    if _m.is_tensor(xyz):
        import torch
        A, t = torch.as_tensor(T[:3, :3], device=xyz.device), torch.as_tensor(T[:3, 3], device=xyz.device)
        return (xyz.detach().double() @ A.T + t).float()
    return (np.asarray(xyz, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


class NonRigidRefiner:
    """``NonRigidRefiner(source_cloud, target_cloud, WarpParams(max_corr=...), init=T).run()`` -> ``WarpResult``.

    The source (a ``PointCloud`` record) is moved by ``init`` (4x4, rigid or a similarity) first.  Then, coarse to fine over lattices
    of ``2^l + 1`` nodes per axis on one box -- ``box`` = ``(lo, hi)``, default ``default_box`` of the moved source -- up to
    ``max_iteration`` times per level: correspondences at the warped positions (nearest target point, strict ``d^2 < max_corr^2``,
    lowest index on a tie), the per-cell sums on the GPU (``gsr_warp_accumulate``), one exact solve on the host (``gsr_warp_solve``).
    A level stops early when the point-to-plane RMSE changes by less than ``relative_rmse`` relatively, or without a correspondence.
    The target's normals are the record's, else estimated as ``PointCloud.estimate_normals`` does.  Only the source moves."""

    def __init__(self, source_cloud, target_cloud, params, init=None, device=None, box=None):
        if params.max_corr is None or not params.max_corr > 0:
            raise ValueError("WarpParams.max_corr must be set and positive")
        if not 1 <= int(params.levels) <= 5:
            raise ValueError("WarpParams.levels must lie in [1, 5] (2^3 .. 17^3 nodes)")
        self.source, self.target, self.params = source_cloud, target_cloud, params
        self.init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4)
        self.device = int(target_cloud.device_index if device is None else device)
        self.box = box

    def _target_normals(self):
        from . import icp
        t = self.target
        if t.has_normals():
            return t.normals
        if t.cov6 is None:
            return icp.normals_knn(t.xyz32, knn=30, device=self.device)
        return icp.normals_from_cov(t.cov6, device=self.device)

    def run(self):
        P = self.params
        t_start = time.perf_counter()
        src = _moved_f32(self.source.xyz32, self.init)
        tgt, nrm = self.target.xyz32, self._target_normals()
        if _is_cuda(tgt) != _is_cuda(nrm):                                  # the normals go where the points live
            import torch
            nrm = torch.as_tensor(np.asarray(nrm), device=tgt.device) if _is_cuda(tgt) else nrm.detach().cpu().numpy()
        lo, hi = self.box if self.box is not None else default_box(src.detach().cpu().numpy() if _m.is_tensor(src) else src)
        res = WarpResult()
        tm = {"build": 0.0, "accumulate": 0.0, "solve": 0.0}
        with WarpContext(self.device) as ctx:
            t0 = time.perf_counter()
            ctx.set_target(tgt, nrm, P.max_corr)
            ctx.set_source(src)
            tm["build"] = time.perf_counter() - t0

            def accumulate(f):
                t0 = time.perf_counter()
                out = ctx.accumulate(f)
                tm["accumulate"] += time.perf_counter() - t0
                return out

            fld = None
            for level in range(int(P.levels)):
                dims = (2 ** level + 1,) * 3
                fld = WarpField(WarpLattice(lo, hi, dims)) if fld is None else fld.prolong(dims)
                its, prev = [], None
                for _ in range(int(P.max_iteration)):
                    sums, n, rmse = accumulate(fld)
                    if not res.levels and not its:
                        res.rmse_before = rmse
                    if n == 0 or (prev is not None and abs(prev - rmse) < P.relative_rmse * prev):
                        break
                    prev = rmse
                    t0 = time.perf_counter()
                    U, rep = solve(dims, sums, P.lam, P.lam0, fld.U)
                    tm["solve"] += time.perf_counter() - t0
                    fld = WarpField(fld.lattice, U)
                    its.append({"n_corr": n, "rmse": rmse, "E_before": rep["E_before"], "E_after": rep["E_after"]})
                res.levels.append({"dims": dims, "iterations": its})
            _, res.n_corr, res.rmse_after = accumulate(fld)
        res.field = fld
        n_src = int(src.shape[0])
        if n_src:
            eye6 = np.tile(np.float32([1, 0, 0, 1, 0, 1]), (n_src, 1))
            if _is_cuda(src):
                import torch
                eye6 = torch.as_tensor(eye6, device=src.device)
            res.n_folded = fld.apply_arrays(src, eye6, device=self.device)[2]
        tm["total"] = time.perf_counter() - t_start
        res.timings = tm
        return res
