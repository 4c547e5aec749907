"""Consistent normal orientation: ctypes front of ``gsr_orient_normals_graph`` and ``gsr_orient_normals`` (``csrc/orient.hip``,
DESIGN.md section 19).

The signs of the normals are propagated along the minimum spanning forest of the neighbour graph (edge weight ``1 - |n_i . n_j|``),
every connected piece then takes the sign most of its normals need to look towards ``reference``.  numpy arrays are staged through
the host by the library and come back as numpy arrays; PyTorch-ROCm tensors on the device stay there.  The input normals are not
modified: the result is a copy.  No GPU: ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as _m

__all__ = ["orient_normals", "orient_normals_graph"]

_PHASES = ("lists", "csr", "rounds", "vote_flip")


def _call(entry, xyz, normals, reference, device, with_component, lists=None, search=None):
    L = _lib.load(require_device=True)
    on = _m.is_cuda(normals)
    if on:
        device = normals.device.index
    n = int(normals.shape[0])
    if on:                                                            # the library writes in place: hand it a copy
        out = normals.detach().double().reshape(n, 3).contiguous().clone()
        p_nrm = out.data_ptr()
    else:
        out = np.array(normals.detach().cpu().numpy() if _m.is_tensor(normals) else normals, dtype=np.float64, order="C").reshape(n, 3)
        p_nrm = out.ctypes.data
    p_xyz, k_xyz, on_xyz = _m.prep(xyz, (n, 3), np.float32, device)
    if on_xyz is not None and on_xyz != on:
        raise RuntimeError("the arrays must all live on the host or all on one device")
    ref = None
    if reference is not None:
        ref = (C.c_double * 3)(*[float(x) for x in np.asarray(reference.detach().cpu() if _m.is_tensor(reference) else reference, np.float64).reshape(3)])
    comp, p_comp = _m.out((n,), np.int32, device, on) if with_component else (None, None)
    R = _lib.OrientReport()
    tail = (ref, p_comp, C.addressof(R), 1 if on else 0, int(device), C.c_void_p(_m.stream_ptr(device, on)))
    if lists is not None:
        nbr, count = lists
        stride = int(nbr.shape[1]) if len(nbr.shape) == 2 else int(np.prod(tuple(nbr.shape))) // max(n, 1)
        p_nbr, k_nbr, on_nbr = _m.prep(nbr, (n, stride), np.int32, device)
        p_cnt, k_cnt, on_cnt = _m.prep(count, (n,), np.int32, device)
        if on_nbr != on or on_cnt != on:
            raise RuntimeError("the lists must live where the normals live")
        _lib.check(L.gsr_orient_normals_graph(p_xyz, p_nrm, n, p_nbr, stride, p_cnt, *tail), entry)
    else:
        radius, max_nn = search
        _lib.check(L.gsr_orient_normals(p_xyz, p_nrm, n, float(radius), int(max_nn), *tail), entry)
    info = {k: int(getattr(R, k)) for k in ("n", "n_components", "n_flipped", "n_not_live", "rounds", "workspace_bytes")}
    info["phase_ms"] = dict(zip(_PHASES, (float(x) for x in R.phase_ms)))      # device events of the call
    if with_component:
        info["component"] = comp
    return out, info


def orient_normals_graph(xyz, normals, nbr, count, reference=None, device=0, with_component=True):
    """Orientation over given neighbour lists (``nbr`` (n, stride) int32, ``count`` (n,) int32: the layout of
    ``features.hybrid_search``) -> ``(normals, info)``.  ``normals`` (n, 3) float64: every row the input or its exact negation;
    ``info``: ``n``, ``n_components``, ``n_flipped``, ``n_not_live``, ``rounds``, ``workspace_bytes``, ``phase_ms`` and
    ``component`` (n,) int32, the lowest vertex of each vertex's connected piece.  ``reference``: a point (3,) the pieces look
    towards, or ``None`` (then the lowest vertex of every piece keeps its sign and ``xyz`` may be ``None``)."""
    return _call("gsr_orient_normals_graph", xyz, normals, reference, device, with_component, lists=(nbr, count))


def orient_normals(xyz, normals, radius, max_nn, reference=None, device=0, with_component=True):
    """The same over the lists of ``KDTreeSearchParamHybrid(radius, max_nn)``, searched on the device."""
    return _call("gsr_orient_normals", xyz, normals, reference, device, with_component, search=(radius, max_nn))
