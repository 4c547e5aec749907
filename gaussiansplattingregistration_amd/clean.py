"""Floater removal: ctypes front of ``gsr_outlier_mask`` and ``gsr_model_select`` (``csrc/clean.hip``).

``outlier_mask`` says which rows of a cloud or splat model survive the finite test, the splat gates, Open3D's statistical
filter and Open3D's radius filter, in that order; ``select_rows`` copies the kept rows of any set of row-major float32 arrays,
bit for bit.  numpy arrays are staged through the host by the library; PyTorch-ROCm tensors on the device are read and written
in place and the results are tensors on that device.  No GPU: ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as _m
from . import _model_view as _mv



def outlier_mask(xyz, params, raw_opacity=None, scaling=None, device=0, with_mean_dist=False, with_count=False):
    """-> ``(mask, info)``: ``mask`` (n,) uint8, 1 = kept; ``info``: the report of ``gsr_outlier_mask`` (rows dropped per stage,
    ``n_kept``, ``cloud_mean`` / ``std_dev`` / ``threshold``, ``deferred_queries``, ``workspace_bytes``, ``phase_ms``) and, when
    asked for, ``mean_dist`` (n,) float64 and ``count`` (n,) int32 (-1 for rows that did not reach the stage).  ``params``: a
    ``CleanParams``; a gate that is on needs its array (``raw_opacity`` (n,), ``scaling`` (n, 3): the stored log-scales)."""
    params.validate()
    L = _lib.load(require_device=True)
    n = int(xyz.shape[0])
    if _m.is_cuda(xyz):
        device = xyz.device.index
    p_xyz, k0, on = _m.prep(xyz, (n, 3), np.float32, device)
    gate_op, gate_sc = params.min_raw_opacity > -np.inf, params.max_log_scale < np.inf
    if gate_op and raw_opacity is None:
        raise ValueError("min_opacity is set but the cloud has no opacities")
    if gate_sc and scaling is None:
        raise ValueError("max_extent is set but the cloud has no scales")
    p_op, k1, on1 = _m.prep(raw_opacity if gate_op else None, (n,), np.float32, device)
    p_sc, k2, on2 = _m.prep(scaling if gate_sc else None, (n, 3), np.float32, device)
    if any(o is not None and o != on for o in (on1, on2)):
        raise RuntimeError("the arrays must all live on the host or all on one device")
    mask, p_mask = _m.out((n,), np.uint8, device, on)
    mean, p_mean = _m.out((n,), np.float64, device, on) if with_mean_dist else (None, None)
    cnt, p_cnt = _m.out((n,), np.int32, device, on) if with_count else (None, None)
    P = _lib.CleanParams(params.min_raw_opacity, params.max_log_scale, int(params.nb_neighbors), 0, float(params.std_ratio), float(params.radius),
                         int(params.nb_points), 0)
    R = _lib.CleanReport()
    _lib.check(L.gsr_outlier_mask(p_xyz, p_op, p_sc, n, C.addressof(P), p_mask, p_mean, p_cnt, C.addressof(R), *_mv.call_tail(device, on)), "gsr_outlier_mask")
    info = {k: int(getattr(R, k)) for k in ("n", "n_nonfinite", "n_gate_opacity", "n_gate_scale", "n_statistical", "n_radius", "n_kept",
                                            "deferred_queries", "workspace_bytes")}
    info.update({k: float(getattr(R, k)) for k in ("cloud_mean", "std_dev", "threshold")})
    info["phase_ms"] = dict(zip(("prepass_grid", "knn", "radius", "mask"), (float(x) for x in R.phase_ms)))      # device events of the call
    if with_mean_dist:
        info["mean_dist"] = mean
    if with_count:
        info["count"] = cnt
    return mask, info


def select_rows(arrays, mask, device=0):
    """The rows with ``mask != 0`` of every array of ``arrays`` (name -> row-major float32 array with n rows, or ``None``), in
    ascending order, bit for bit -> ``(selected, index)``: name -> array with ``n_kept`` rows (trailing shape kept) and the kept
    input rows (n_kept,) int32 -- Open3D's second return value.  The names are the fields of ``gsr_model_view`` (``xyz``, ``cov6``,
    ``dc``, ``sh``, ``opacity``, ``scaling``, ``rot``): ``sh`` has 3K floats per row, K in {0, 3, 8, 15}; ``scaling`` and ``rot``
    come both or neither.  One library call for all arrays."""
    L = _lib.load(require_device=True)
    unknown = set(arrays) - {field for field, _, _ in _mv.FIELDS}
    if unknown:
        raise ValueError(f"unknown arrays {sorted(unknown)}")
    given = {k: a for k, a in arrays.items() if a is not None}
    if not given:
        raise ValueError("no array to select from")
    n = int(next(iter(given.values())).shape[0])
    first = next(iter(given.values()))
    if _m.is_cuda(first):
        device = first.device.index
    on = _m.is_cuda(first)
    K = 0
    if "sh" in given:
        w = int(np.prod(tuple(given["sh"].shape[1:])))
        if w % 3:
            raise ValueError("sh must hold 3K floats per row")
        K = w // 3
    vin, vout, keep, outs, shapes = _lib.ModelView(), _lib.ModelView(), [], {}, {}
    vin.n, vout.n = n, n
    for name, _, width in _mv.carried(K, True, fields=given):          # (K = 0: sh is not carried)
        a = given[name]
        if int(a.shape[0]) != n:
            raise ValueError(f"{name}: {a.shape[0]} rows, expected {n}")
        p, k, a_on = _m.prep(a, (n, width), np.float32, device)
        if a_on != on:
            raise RuntimeError("the arrays must all live on the host or all on one device")
        keep.append(k)
        setattr(vin, name, p)
        outs[name], po = _m.out((n, width), np.float32, device, on)
        setattr(vout, name, po)
        shapes[name] = tuple(a.shape[1:])
    p_mask, km, m_on = _m.prep(mask, (n,), np.uint8, device)
    if n > 0 and m_on != on:
        raise RuntimeError("the mask must live where the arrays live")
    index, p_index = _m.out((n,), np.int32, device, on)
    n_out = C.c_int64(0)
    _lib.check(L.gsr_model_select(C.addressof(vin), K, p_mask, C.addressof(vout), p_index, C.byref(n_out), *_mv.call_tail(device, on)), "gsr_model_select")
    m = int(n_out.value)
    return {name: o[:m].reshape((m,) + shapes[name]) for name, o in outs.items()}, index[:m]


def add_clean_arguments(ap):
    """the cleaning flags the command-line tools share (scripts/clean_ply.py, register_ply.py, register_many.py)"""
    ap.add_argument("--clean-knn", type=int, metavar="K", help="floater removal: neighbours of the statistical filter (with --clean-std)")
    ap.add_argument("--clean-std", type=float, metavar="R", help="floater removal: std_ratio of the statistical filter")
    ap.add_argument("--clean-radius", type=float, metavar="R", help="floater removal: radius of the radius filter (with --clean-nb)")
    ap.add_argument("--clean-nb", type=int, metavar="N", help="floater removal: a splat needs more than N splats within --clean-radius")
    ap.add_argument("--clean-min-opacity", type=float, metavar="A", help="floater removal: drop splats whose opacity is below A")
    ap.add_argument("--clean-max-extent", type=float, metavar="S", help="floater removal: drop splats whose largest scale exceeds S")


def add_prune_arguments(ap):
    """the visibility-pruning flags the command-line tools share (``GaussianModel.prune_unseen``)"""
    ap.add_argument("--prune-unseen", action="append", metavar="CAMERAS.json", help="drop the splats no camera of these files shows with a blending "
                    "weight of --min-contribution (may be given several times: pass the cameras of ALL merged scenes, a splat outside every "
                    "frustum is dropped like an occluded one)")
    ap.add_argument("--min-contribution", type=float, default=0.01, help="smallest largest blending weight alpha T of a kept splat (RadSplat: 0.01)")


def prune_unseen_from_args(model, a, report=print):
    """``model`` without the splats the cameras of ``--prune-unseen`` never show (the model itself when the flag is absent)"""
    if not a.prune_unseen:
        return model
    from .models.camera import load_cameras
    cameras = [c for path in a.prune_unseen for c in load_cameras(path)]
    pruned, info = model.prune_unseen(cameras, min_contribution=a.min_contribution)
    report(f"prune unseen: {len(cameras)} cameras, {info['n']} -> {info['n_kept']} splats (largest blending weight below {a.min_contribution:g} dropped)")
    return pruned


def clean_params_from_args(a):
    """-> ``CleanParams`` or ``None`` when no cleaning flag was given"""
    from .params.clean_parameters import CleanParams
    flags = (a.clean_knn, a.clean_std, a.clean_radius, a.clean_nb, a.clean_min_opacity, a.clean_max_extent)
    if all(f is None for f in flags):
        return None
    if (a.clean_knn is None) != (a.clean_std is None):
        raise SystemExit("--clean-knn and --clean-std come together")
    if (a.clean_radius is None) != (a.clean_nb is None):
        raise SystemExit("--clean-radius and --clean-nb come together")
    try:
        return CleanParams(min_opacity=a.clean_min_opacity or 0.0, max_extent=a.clean_max_extent if a.clean_max_extent is not None else float("inf"),
                           nb_neighbors=a.clean_knn or 0, std_ratio=a.clean_std if a.clean_std is not None else 2.0,
                           radius=a.clean_radius or 0.0, nb_points=a.clean_nb if a.clean_nb is not None else 16)
    except ValueError as e:
        raise SystemExit(str(e))
