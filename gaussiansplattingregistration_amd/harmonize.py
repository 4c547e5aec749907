"""Colour harmonisation of registered scenes: ctypes front of ``gsr_model_match``, ``gsr_color_sums``, ``gsr_color_solve`` and
``gsr_model_color_apply`` (``csrc/fuse.hip``, ``csrc/harmonize.hip``, ``csrc/gsr_colorsolve.h``).

Scenes trained from separate captures differ in exposure and white balance.  ``match_pairs`` finds the splats two registered models
share (the mutual-best-match rule of the overlap-aware merge, without its writer), ``color_sums`` reduces the matched pairs of one
edge to 39 float64 sums at the current transforms, ``solve_colors`` fits the transforms of all scenes jointly from the sums of all
edges, and ``apply_colors`` rewrites a model's DC and SH coefficients.  ``match_colors`` is the whole loop.  numpy arrays are staged
through the host by the library; PyTorch-ROCm tensors on the device are used in place.  No GPU: ``RuntimeError`` (``solve_colors``
alone is host code and needs none).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from . import _marshal as _m
from . import _model_view as _mv

C0 = 0.28209479177387814
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def match_pairs(model_a, model_b, fuse_params):
    """-> ``(pairs, report)``: the pair list ``GaussianModel.fuse_overlap(model_a, model_b, fuse_params)`` would fuse -- (n_pairs, 2)
    int32, row of ``model_a`` and row of ``model_b``, ascending in the first -- without building a model (``gsr_model_match``).
    ``report``: ``n_pairs``, ``n_out`` (what the fusion would return), ``n_a_only``, ``n_b_only``, ``n_invalid_a``, ``n_invalid_b``,
    ``gated_pairs``, ``workspace_bytes``, ``phase_ms``.  The two models must be in one frame and on one device."""
    L = _lib.load(require_device=True)
    on, device = _mv.placement([model_a, model_b])
    keep = []
    va, vb = (_mv.view_of(g, 0, False, device, on, keep, fields=("xyz", "cov6", "dc", "opacity")) for g in (model_a, model_b))
    pairs, ppairs = _m.out((min(len(model_a), len(model_b)), 2), np.int32, device, on)
    P = _lib.FuseParams(float(fuse_params.max_distance), float(fuse_params.kld_max), float(fuse_params.color_delta))
    R = _lib.FuseReport()
    _lib.check(L.gsr_model_match(C.addressof(va), C.addressof(vb), C.addressof(P), ppairs, C.addressof(R), *_mv.call_tail(device, on)), "gsr_model_match")
    info = {k: int(getattr(R, k)) for k in ("n_out", "n_pairs", "n_a_only", "n_b_only", "n_invalid_a", "n_invalid_b", "gated_pairs", "workspace_bytes")}
    info["phase_ms"] = dict(zip(("prepass_grid", "search", "pair_scan"), (float(x) for x in R.phase_ms)))
    return pairs[:info["n_pairs"]], info


def _p12(P):
    P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(3, 4))
    return P


def color_sums(s_dc, s_opacity, t_dc, t_opacity, pairs, P_s=IDENTITY, P_t=IDENTITY, huber=math.inf, device=0):
    """The sums of one edge over its matched pairs (``gsr_color_sums``) -> ``(sums, info)``: ``sums`` (40,) float64 -- n, sum w,
    sum w rho^2, S_aa (upper triangle), S_ab, S_bb (upper triangle), 0 -- and ``info`` with ``n_skipped`` (pairs with a non-finite
    colour or opacity) and ``n_out_of_range`` (0: a pair that indexes a row outside its model raises ``RuntimeError``).
    ``s_dc`` (ns, 3), ``s_opacity`` (ns,) RAW, likewise for the target; ``pairs`` (n_pairs, 2) int32."""
    L = _lib.load(require_device=True)
    ns, nt = int(s_dc.shape[0]), int(t_dc.shape[0])
    n_pairs = int(pairs.shape[0])
    if _m.is_cuda(s_dc):
        device = s_dc.device.index
    on = _m.is_cuda(s_dc)
    ptr, keep = [], []
    for a, shape, dtype in ((s_dc, (ns, 3), np.float32), (s_opacity, (ns,), np.float32), (t_dc, (nt, 3), np.float32), (t_opacity, (nt,), np.float32),
                            (pairs, (n_pairs, 2), np.int32)):
        p, k, a_on = _m.prep(a, shape, dtype, device)
        if a_on != on and shape[0] > 0:
            raise RuntimeError("the arrays must all live on the host or all on one device")
        ptr.append(p)
        keep.append(k)
    Ps, Pt = _p12(P_s), _p12(P_t)
    sums = np.zeros(_lib.GSR_COLOR_SUMS_LEN, np.float64)
    skipped, outside = C.c_int64(0), C.c_int64(0)
    _lib.check(L.gsr_color_sums(ptr[0], ptr[1], ns, ptr[2], ptr[3], nt, ptr[4], n_pairs, Ps.ctypes.data, Pt.ctypes.data, float(huber), sums.ctypes.data,
                                C.byref(skipped), C.byref(outside), *_mv.call_tail(device, on)), "gsr_color_sums")
    return sums, {"n_skipped": int(skipped.value), "n_out_of_range": int(outside.value)}


def solve_colors(P, edges, sums, mode="affine", prior=1e-4, min_pairs=100, reference=0):
    """The joint fit (``gsr_color_solve``; host code) -> ``(P_new, info)``.  ``P`` (N, 3, 4): the transforms the sums were taken
    at -- held nodes keep theirs; ``edges``: E pairs ``(source, target)``; ``sums`` (E, 40) from ``color_sums``.  ``info``: ``held``
    (N,) bool, ``E_initial``, ``E_final``, ``pivot_min``, ``pivot_max``, ``n_free``, ``n_unknowns``.  A bad graph, a non-finite
    value or a singular system (``prior=0`` and pairs that do not determine the mode) raise ``RuntimeError``."""
    L = _lib.load()
    P = np.array(P, dtype=np.float64).reshape(-1, 3, 4)
    N = P.shape[0]
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, _lib.GSR_COLOR_SUMS_LEN)
    edges = [(int(s), int(t)) for s, t in edges]
    if len(edges) != sums.shape[0]:
        raise ValueError(f"{len(edges)} edges and {sums.shape[0]} rows of sums")
    if mode not in _lib.GSR_COLOR_MODES:
        raise ValueError(f"mode {mode!r} (gain, channel_gain or affine)")
    E = (_lib.ColorEdge * max(len(edges), 1))()
    for k, (s, t) in enumerate(edges):
        E[k].source, E[k].target = s, t
        E[k].sums[:] = sums[k].tolist()
    held = np.zeros(N, np.int32)
    R = _lib.ColorSolveResult()
    _lib.check(L.gsr_color_solve(N, P.ctypes.data, len(edges), C.addressof(E), _lib.GSR_COLOR_MODES[mode], float(prior), int(min_pairs), int(reference),
                                 held.ctypes.data, C.addressof(R)), "gsr_color_solve")
    info = {"held": held.astype(bool), "E_initial": float(R.E_initial), "E_final": float(R.E_final), "pivot_min": float(R.pivot_min),
            "pivot_max": float(R.pivot_max), "n_free": int(R.n_free), "n_unknowns": int(R.n_unknowns)}
    return P, info


def apply_color_arrays(P, dc, sh=None, inplace=False, device=0):
    """``x' = M x + b`` on the colour arrays of a model (``gsr_model_color_apply``) -> ``(dc', sh')``: ``dc`` (n, 3) or (n, 1, 3),
    ``sh`` (n, K, 3) with K in {0, 3, 8, 15} or ``None``.  ``inplace``: the arrays themselves are rewritten (they must be contiguous
    float32) and returned."""
    L = _lib.load(require_device=True)
    n = int(dc.shape[0])
    K = int(sh.shape[1]) if sh is not None and sh.ndim == 3 else 0
    if _m.is_cuda(dc):
        device = dc.device.index
    on = _m.is_cuda(dc)
    p_dc, k_dc, _ = _m.prep(dc, (n, 3), np.float32, device)
    p_sh, k_sh, sh_on = _m.prep(sh if K else None, (n, K, 3), np.float32, device)
    if K and n and sh_on != on:
        raise RuntimeError("the arrays must all live on the host or all on one device")
    if inplace:
        same = lambda a, p: (a.data_ptr() if _m.is_tensor(a) else a.ctypes.data) == p
        if not same(dc, p_dc) or (K and not same(sh, p_sh)):
            raise ValueError("inplace needs contiguous float32 arrays")
        o_dc, po_dc, o_sh, po_sh = dc, p_dc, sh, p_sh
    else:
        o_dc, po_dc = _m.out(tuple(dc.shape), np.float32, device, on)
        o_sh, po_sh = _m.out((n, K, 3), np.float32, device, on) if K else (sh, None)
    X = _p12(P)
    _lib.check(L.gsr_model_color_apply(X.ctypes.data, n, K, p_dc, p_sh, po_dc, po_sh, *_mv.call_tail(device, on)), "gsr_model_color_apply")
    return o_dc, o_sh


def apply_colors(model, P, inplace=False):
    """``model`` with the colour transform ``P`` (3, 4) applied to ``_features_dc`` and ``_features_rest`` -> a model (``model``
    itself when ``inplace``).  Everything else is shared with ``model``: geometry and opacity are not touched, colours not clamped."""
    import torch
    K = _mv.sh_count(model)
    m = model
    if not inplace:
        m = type(model)(model.device_name)
        m.sh_degree = model.sh_degree
        for name in ("_xyz", "_scaling", "_rotation", "_opacity", "_covariance", "_features_rest"):
            setattr(m, name, getattr(model, name))
    if len(model) == 0:
        m._features_dc = model._features_dc
        return m
    if inplace and not (model._features_dc.is_contiguous() and (K == 0 or model._features_rest.is_contiguous())):
        model._features_dc = model._features_dc.contiguous()
        model._features_rest = model._features_rest.contiguous()
    dc, sh = apply_color_arrays(P, model._features_dc, model._features_rest if K else None, inplace=inplace)
    m._features_dc = torch.as_tensor(dc)
    if K:
        m._features_rest = torch.as_tensor(sh)
    return m


def match_colors(models, fuse_params, params=None, edges="all", reference=0):
    """The colour transforms that bring N models, ALREADY IN ONE FRAME, into agreement with ``models[reference]`` ->
    ``(transforms, info)``: N arrays (3, 4) float64 (``[I|0]`` for the reference and for every held model) and ``info`` with
    ``edges`` (per edge: ``source``, ``target``, ``n_pairs``, ``n_used``, ``n_skipped``, ``rms_before``, ``rms_after`` -- the weighted
    RMS colour residual at the identity and at the result), ``held`` (N,) bool and ``solve`` (the last solve's report).
    ``fuse_params`` (``FuseOverlapParams``) gates the correspondences; ``params``: a ``ColorMatchParams``; ``edges``: ``"all"``
    (every pair s < t) or a list of ``(s, t)``.  The pair lists are made once; then ``params.iterations`` rounds of: the sums of every
    edge at the current transforms, the joint solve."""
    from .params.merge_parameters import ColorMatchParams
    params = (params or ColorMatchParams()).validate()
    models = list(models)
    N = len(models)
    if N < 1 or not 0 <= reference < N:
        raise ValueError(f"{N} models, reference {reference}")
    if isinstance(edges, str):
        if edges != "all":
            raise ValueError(f"edges {edges!r} ('all' or a list of (s, t))")
        edges = [(s, t) for s in range(N) for t in range(s + 1, N)]
    edges = [(int(s), int(t)) for s, t in edges]
    for s, t in edges:
        if not (0 <= s < N and 0 <= t < N) or s == t:
            raise ValueError(f"edge ({s}, {t}) of {N} models")
    cols = [(g._features_dc.reshape(len(g), 3), g._opacity.reshape(len(g))) for g in models]
    lists, per_edge = [], []
    for s, t in edges:
        pairs, rep = match_pairs(models[s], models[t], fuse_params)
        lists.append(pairs)
        per_edge.append({"source": s, "target": t, "n_pairs": rep["n_pairs"]})
    P = np.tile(IDENTITY, (N, 1, 1))

    def all_sums(P):
        S = np.zeros((len(edges), _lib.GSR_COLOR_SUMS_LEN))
        skipped = []
        for k, (s, t) in enumerate(edges):
            S[k], i = color_sums(cols[s][0], cols[s][1], cols[t][0], cols[t][1], lists[k], P[s], P[t], params.huber)
            skipped.append(i["n_skipped"])
        return S, skipped

    rms = lambda S: [math.sqrt(r[2] / r[1]) if r[1] > 0 else 0.0 for r in S]
    solve = {"held": np.ones(N, bool)}
    first = None
    for _ in range(params.iterations):
        S, skipped = all_sums(P)
        if first is None:
            first = S
        P, solve = solve_colors(P, edges, S, params.mode, params.prior, params.min_pairs, reference)
    last, skipped = all_sums(P)
    for e, r0, r1, S0, sk in zip(per_edge, rms(first), rms(last), first, skipped):
        e.update(n_used=int(S0[0]), n_skipped=sk, rms_before=r0, rms_after=r1)
    return [P[i].copy() for i in range(N)], {"edges": per_edge, "held": solve["held"], "solve": {k: v for k, v in solve.items() if k != "held"}}


def is_identity(P):
    return np.array_equal(np.asarray(P, dtype=np.float64).reshape(3, 4), IDENTITY)


def add_match_colors_arguments(ap):
    """the colour flags the command-line tools share (scripts/register_ply.py, register_many.py, evaluate_registration.py)"""
    ap.add_argument("--match-colors", nargs="?", const="affine", choices=("gain", "channel_gain", "affine"), metavar="MODE",
                    help="harmonise the colours of the scenes before merging: gain (exposure), channel_gain (white balance) or affine (default)")
    ap.add_argument("--match-colors-huber", type=float, default=0.1, metavar="K", help="Huber threshold on the colour residual (default 0.1)")
    ap.add_argument("--match-colors-dist", type=float, metavar="D", help="largest distance between matched splat centres (default: the fuse distance)")
    ap.add_argument("--colors-out", metavar="colors.json", help="write the colour transforms and residuals here")


def match_colors_from_args(a, fuse=None, default_distance=None):
    """-> ``(ColorMatchParams, FuseOverlapParams gate)`` or ``(None, None)`` when ``--match-colors`` was not given"""
    from .params.merge_parameters import ColorMatchParams, FuseOverlapParams
    if a.match_colors is None:
        return None, None
    dist = a.match_colors_dist if a.match_colors_dist is not None else (fuse.max_distance if fuse is not None else default_distance)
    if dist is None:
        raise SystemExit("--match-colors needs --match-colors-dist (or a fuse distance)")
    gate = FuseOverlapParams(max_distance=dist) if (fuse is None or a.match_colors_dist is not None) else fuse
    return ColorMatchParams(mode=a.match_colors, huber=a.match_colors_huber), gate


def report_lines(transforms, info):
    """what the command-line tools print per scene and edge"""
    lines = []
    for i, P in enumerate(transforms):
        tag = " (held)" if info["held"][i] else ""
        lines.append(f"scene {i}{tag}: " + "; ".join(" ".join(f"{v:+.4f}" for v in row) for row in np.asarray(P)))
    for e in info["edges"]:
        lines.append(f"edge {e['source']} -> {e['target']}: {e['n_pairs']} pairs, {e['n_used']} used, colour rms {e['rms_before']:.4f} -> {e['rms_after']:.4f}")
    return lines


def write_json(path, transforms, info):
    import json
    with open(path, "w") as f:
        json.dump({"transforms": [np.asarray(P).tolist() for P in transforms], "held": [bool(h) for h in info["held"]], "edges": info["edges"],
                   "solve": info["solve"]}, f, indent=1)
