"""Global registration on the GPU: ctypes front of ``gsr_hybrid_search``, ``gsr_fpfh``, ``gsr_feature_match``,
``gsr_ransac_correspondence`` (``csrc/features.hip``), ``gsr_fgr_tuple_test`` and ``gsr_fgr_optimize`` (``csrc/fgr.hip``) and
``gsr_sc2_correspondence`` (``csrc/sc2.hip``), all declared in ``include/gsr_hip.h``.

Reference behaviour: ``compute_fpfh_feature``, ``registration_ransac_based_on_feature_matching`` and
``registration_fgr_based_on_feature_matching`` of Open3D 0.16.0 as the reference's ``src/utils/global_registration_util.py`` calls
them.  Inputs are numpy arrays or cuda tensors (all on the host or
all on the device); ``as_torch`` returns cuda tensors the library wrote in place.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as _m

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["hybrid_search", "fpfh", "feature_match", "ransac_correspondence", "fgr_tuple_test", "fgr_optimize", "sc2_correspondence", "KIND_POINT_TO_POINT",
           "KIND_POINT_TO_PLANE",
           "CHECK_EDGE_LENGTH", "CHECK_DISTANCE", "CHECK_NORMAL"]

KIND_POINT_TO_POINT = 0
KIND_POINT_TO_PLANE = 1
KIND_POINT_TO_POINT_SCALED = 4          # Umeyama with scaling: the hypotheses are similarities
CHECK_EDGE_LENGTH = _lib.GSR_CHECK_EDGE_LENGTH
CHECK_DISTANCE = _lib.GSR_CHECK_DISTANCE
CHECK_NORMAL = _lib.GSR_CHECK_NORMAL


def _rows(a, cols, dtype, device, on_device):
    """-> (pointer, keep-alive, n) of a contiguous (n, cols) array of `dtype`, which must lie where `on_device` says"""
    p, keep, on = _m.prep(a, (-1, cols), dtype, device)
    if on is not None and on != bool(on_device):
        raise RuntimeError("inputs must be all on the host or all on the device")
    return p, keep, 0 if keep is None else int(keep.shape[0])


def hybrid_search(xyz, radius, max_nn, device=0):
    """``KDTreeSearchParamHybrid(radius, max_nn)`` of every point against the cloud: ``(nbr (n, max_nn) int32, count (n,) int32)``;
    row i lists ``count[i]`` input indices in (d2, index) order (the rest of the row is unspecified)."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(xyz)
    px, kx, n = _rows(xyz, 3, np.float32, device, on)
    nbr, pn = _m.out((n, int(max_nn)), np.int32, device, on)
    cnt, pc = _m.out((n,), np.int32, device, on)
    _lib.check(L.gsr_hybrid_search(px, n, float(radius), int(max_nn), pn, pc, 1 if on else 0, int(device), C.c_void_p(_m.stream_ptr(device, on))),
               "gsr_hybrid_search")
    return nbr, cnt


def fpfh(xyz, normals, radius, max_nn, device=0, as_torch=False):
    """Open3D ``ComputeFPFHFeature``: float64 (n, 33) rows (numpy, or a cuda tensor when the inputs are on the device or
    ``as_torch``)."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(xyz)
    if as_torch and not on:
        xyz = torch.as_tensor(np.asarray(xyz, np.float32)).to(torch.device("cuda", device))
        normals = torch.as_tensor(np.asarray(normals, np.float64)).to(torch.device("cuda", device))
        on = True
    px, kx, n = _rows(xyz, 3, np.float32, device, on)
    pn, kn, nn = _rows(normals, 3, np.float64, device, on)
    if normals is None or nn != n:
        raise RuntimeError("[Open3D Error] ComputeFPFHFeature needs one normal per point")
    out, po = _m.out((n, 33), np.float64, device, on)
    _lib.check(L.gsr_fpfh(px, pn, n, float(radius), int(max_nn), po, 1 if on else 0, int(device), C.c_void_p(_m.stream_ptr(device, on))), "gsr_fpfh")
    return out


def feature_match(src_feat, tgt_feat, mutual=False, ransac_n=3, device=0, return_nn=False):
    """Correspondences of ``registration_ransac_based_on_feature_matching``: ``corres (m, 2) int32`` (the mutual set when
    ``mutual`` and it holds >= 3 * ransac_n pairs, else every (i, nn(i))) and whether the mutual set was used; with ``return_nn``
    also the two nearest-row arrays (``nn_ts`` is None without ``mutual``)."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(src_feat)
    pa, ka, ns = _rows(src_feat, 33, np.float64, device, on)
    pb, kb, nt = _rows(tgt_feat, 33, np.float64, device, on)
    corres, pcor = _m.out((ns, 2), np.int32, device, on)
    nst, pst = _m.out((ns,), np.int32, device, on)
    nts, pts = _m.out((nt,), np.int32, device, on) if mutual else (None, None)
    m = C.c_int64(0)
    um = C.c_int32(0)
    _lib.check(L.gsr_feature_match(pa, ns, pb, nt, 1 if mutual else 0, int(ransac_n), pcor, C.byref(m), C.byref(um), pst, pts,
                                   1 if on else 0, int(device), C.c_void_p(_m.stream_ptr(device, on))), "gsr_feature_match")
    corres = corres[: int(m.value)]
    if return_nn:
        return corres, bool(um.value), nst, nts
    return corres, bool(um.value)


def ransac_correspondence(src_xyz, tgt_xyz, corres, max_corr, kind=KIND_POINT_TO_POINT, ransac_n=3, checkers=(), max_iteration=100000,
                          confidence=0.999, seed=0, batch=8192, src_normals=None, tgt_normals=None, device=0):
    """Open3D ``RegistrationRANSACBasedOnCorrespondence``, deterministic (``include/gsr_hip.h``).  ``checkers``: sequence of
    (CHECK_*, parameter).  Returns a dict: transformation, fitness, inlier_rmse, best_index, n_evaluated, n_valid, exit_index."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(src_xyz)
    ps, ks, ns = _rows(src_xyz, 3, np.float32, device, on)
    pt, kt, nt = _rows(tgt_xyz, 3, np.float32, device, on)
    pc, kc, m = _rows(corres, 2, np.int32, device, on)
    psn, ksn, _ = _rows(src_normals, 3, np.float64, device, on)
    ptn, ktn, _ = _rows(tgt_normals, 3, np.float64, device, on)
    checkers = list(checkers)
    if len(checkers) > 4:
        raise RuntimeError("at most 4 correspondence checkers")
    P = _lib.RansacParams()
    P.kind, P.ransac_n, P.max_corr, P.max_iteration = int(kind), int(ransac_n), float(max_corr), int(max_iteration)
    P.confidence, P.seed, P.batch, P.n_checkers = float(confidence), int(seed) & ((1 << 64) - 1), int(batch), len(checkers)
    for i, (ck, cp) in enumerate(checkers):
        P.checker_kind[i] = int(ck)
        P.checker_param[i] = float(cp)
    R = _lib.RansacResult()
    _lib.check(L.gsr_ransac_correspondence(ps, ns, pt, nt, psn, ptn, pc, m, C.byref(P), C.byref(R), 1 if on else 0, int(device),
                                           C.c_void_p(_m.stream_ptr(device, on))), "gsr_ransac_correspondence")
    return {"transformation": np.array(R.T[:], dtype=np.float64).reshape(4, 4), "fitness": R.fitness, "inlier_rmse": R.inlier_rmse,
            "best_index": int(R.best_index), "n_evaluated": int(R.n_evaluated), "n_valid": int(R.n_valid), "exit_index": int(R.exit_index)}


def _sc2_params(d_thr, seed_ratio, max_seeds, k1, k2, refine_iters):
    P = _lib.Sc2Params()
    P.d_thr, P.seed_ratio, P.max_seeds = float(d_thr), float(seed_ratio), int(max_seeds)
    P.k1, P.k2, P.refine_iters = int(k1), int(k2), int(refine_iters)
    return P


def _sc2_dict(R):
    return {"transformation": np.array(R.T[:], dtype=np.float64).reshape(4, 4), "fitness": R.fitness, "inlier_rmse": R.inlier_rmse,
            "best_seed": int(R.best_seed), "best_index": int(R.best_index), "n_seeds": int(R.n_seeds), "n_valid": int(R.n_valid),
            "n_edges": int(R.n_edges), "refine_steps": int(R.refine_steps), "host_waits": int(R.host_waits)}


def sc2_correspondence(src_xyz, tgt_xyz, corres, d_thr, seed_ratio=0.2, max_seeds=4096, k1=30, k2=20, refine_iters=20, device=0):
    """Compatibility-graph global registration over ``corres (m, 2)`` (``gsr_sc2_correspondence``, ``include/gsr_hip.h``): rigid,
    deterministic, no sampling.  Returns a dict: transformation (source -> target), fitness, inlier_rmse, best_seed (rank), best_index
    (correspondence), n_seeds, n_valid, n_edges, refine_steps, host_waits."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(src_xyz)
    ps, ks, ns = _rows(src_xyz, 3, np.float32, device, on)
    pt, kt, nt = _rows(tgt_xyz, 3, np.float32, device, on)
    pc, kc, m = _rows(corres, 2, np.int32, device, on)
    P = _sc2_params(d_thr, seed_ratio, max_seeds, k1, k2, refine_iters)
    R = _lib.Sc2Result()
    _lib.check(L.gsr_sc2_correspondence(ps, ns, pt, nt, pc, m, C.byref(P), C.byref(R), 1 if on else 0, int(device),
                                        C.c_void_p(_m.stream_ptr(device, on))), "gsr_sc2_correspondence")
    return _sc2_dict(R)


def _fgr_options(division_factor=1.4, use_absolute_scale=False, decrease_mu=False, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, seed=0, batch=0):
    O = _lib.FgrOptions()
    O.division_factor, O.use_absolute_scale, O.decrease_mu = float(division_factor), int(bool(use_absolute_scale)), int(bool(decrease_mu))
    O.maximum_correspondence_distance, O.iteration_number = float(maximum_correspondence_distance), int(iteration_number)
    O.maximum_tuple_count, O.tuple_scale, O.tuple_test = int(maximum_tuple_count), float(tuple_scale), int(bool(tuple_test))
    O.batch, O.seed = int(batch), int(seed) & ((1 << 64) - 1)
    return O


def fgr_tuple_test(src_xyz, tgt_xyz, corres, tuple_scale=0.95, maximum_tuple_count=1000, seed=0, batch=0, device=0):
    """The tuple test of Fast Global Registration over ``corres (m, 2)`` (``gsr_fgr_tuple_test``): ``(pairs (3 * accepted, 2) int32,
    n_trials)``, the accepted triples in trial order, at most ``maximum_tuple_count`` of them.  ``batch`` (0: the library's default)
    is a speed knob only."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(src_xyz)
    ps, ks, ns = _rows(src_xyz, 3, np.float32, device, on)
    pt, kt, nt = _rows(tgt_xyz, 3, np.float32, device, on)
    pc, kc, m = _rows(corres, 2, np.int32, device, on)
    O = _fgr_options(tuple_scale=tuple_scale, maximum_tuple_count=maximum_tuple_count, seed=seed, batch=batch)
    out, po = _m.out((3 * max(int(maximum_tuple_count), 0), 2), np.int32, device, on)
    n_out, n_trials = C.c_int64(0), C.c_int64(0)
    _lib.check(L.gsr_fgr_tuple_test(ps, ns, pt, nt, pc, m, C.byref(O), po, C.byref(n_out), C.byref(n_trials), 1 if on else 0, int(device),
                                    C.c_void_p(_m.stream_ptr(device, on))), "gsr_fgr_tuple_test")
    return out[: int(n_out.value)], int(n_trials.value)


def fgr_optimize(src_xyz, tgt_xyz, corres, division_factor=1.4, use_absolute_scale=False, decrease_mu=False,
                 maximum_correspondence_distance=0.025, iteration_number=64, device=0):
    """Normalisation, graduated-non-convexity optimisation and the way back of Fast Global Registration over ``corres (m, 2)``
    (``gsr_fgr_optimize``).  Returns a dict: transformation (source -> target), n_corres, iterations, scale_global, host_waits."""
    L = _lib.load(require_device=True)
    on = _m.is_cuda(src_xyz)
    ps, ks, ns = _rows(src_xyz, 3, np.float32, device, on)
    pt, kt, nt = _rows(tgt_xyz, 3, np.float32, device, on)
    pc, kc, m = _rows(corres, 2, np.int32, device, on)
    O = _fgr_options(division_factor, use_absolute_scale, decrease_mu, maximum_correspondence_distance, iteration_number)
    R = _lib.FgrResult()
    _lib.check(L.gsr_fgr_optimize(ps, ns, pt, nt, pc, m, C.byref(O), C.byref(R), 1 if on else 0, int(device),
                                  C.c_void_p(_m.stream_ptr(device, on))), "gsr_fgr_optimize")
    return {"transformation": np.array(R.T[:], dtype=np.float64).reshape(4, 4), "n_corres": int(R.n_corres), "iterations": int(R.iterations),
            "scale_global": float(R.scale_global), "host_waits": int(R.host_waits)}
