"""A splat model as ``gsr_model_view``: the seven arrays, their widths and which of them a call carries -- the Python side of
``csrc/gsr_model_arrays.h``.  The fronts that hand whole models to the library (``fuse_overlap``, ``fuse_overlap_multi``,
``select_by_mask``, ``harmonize.match_pairs``) build their views and their result models here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as _m

# (field of gsr_model_view, attribute of GaussianModel, floats per row; None: 3 K)
FIELDS = (("xyz", "_xyz", 3), ("cov6", "_covariance", 6), ("dc", "_features_dc", 3), ("sh", "_features_rest", None), ("opacity", "_opacity", 1),
          ("scaling", "_scaling", 3), ("rot", "_rotation", 4))
ATTRS = tuple(attr for _, attr, _ in FIELDS)


def carried(K, with_sr, fields=None):
    """-> [(field, attribute, width)] of the arrays a call with K SH coefficients, with or without scaling / rot, carries"""
    return [(f, a, 3 * K if w is None else w) for f, a, w in FIELDS
            if (f != "sh" or K > 0) and (f not in ("scaling", "rot") or with_sr) and (fields is None or f in fields)]


def sh_count(model):
    """K: SH coefficients per channel beyond the DC term"""
    return int(model._features_rest.shape[1]) if model._features_rest.dim() == 3 else 0


def has_scaling_rot(model):
    return model._scaling.numel() > 0 and model._rotation.numel() > 0


def placement(models):
    """-> (on, device): on one CUDA device, or all on the host (device 0 runs the call)"""
    first = models[0]._xyz
    on = bool(first.is_cuda)
    if any(bool(g._xyz.is_cuda) != on or (on and g._xyz.device != first.device) for g in models):
        raise RuntimeError("the models must all live on one device")
    return on, (first.device.index if on else 0)


def layout(models):
    """-> (K, with_sr) of models that go into one call: one K, and one set of arrays among the models that have rows"""
    Ks = [sh_count(g) for g in models]
    if any(g.sh_degree != models[0].sh_degree for g in models) or any(k != Ks[0] for k in Ks):
        raise RuntimeError("the models carry different numbers of SH coefficients")
    have = [has_scaling_rot(g) for g in models if len(g) > 0]
    if have and any(h != have[0] for h in have):
        raise RuntimeError("_scaling / _rotation: some models carry them, others do not")
    return Ks[0], bool(have and have[0])


def view_of(model, K, with_sr, device, on, keep, fields=None):
    """-> ``ModelView`` of the model's own arrays (of ``fields`` only, when given); a model without rows carries none.  What must
    outlive the call is appended to ``keep``."""
    n = len(model)
    v = _lib.ModelView()
    v.n = n
    for field, attr, width in carried(K, with_sr, fields) if n else ():
        p, k, t_on = _m.prep(getattr(model, attr), (n, width), np.float32, device)
        if t_on != on:
            raise RuntimeError("the model's tensors must all live on one device")
        keep.append(k)
        setattr(v, field, p)
    return v


def out_view(rows, K, with_sr, device, on):
    """-> (``ModelView`` of fresh arrays of ``rows`` rows for the library to write, attribute -> array)"""
    v, arrays = _lib.ModelView(), {}
    v.n = rows
    for field, attr, width in carried(K, with_sr):
        arrays[attr], p = _m.out((rows, width), np.float32, device, on)
        setattr(v, field, p)
    return v, arrays


def model_from_arrays(arrays, n_out, K, sh_degree, device_name):
    """-> a ``GaussianModel`` on the first ``n_out`` rows of ``arrays`` (attribute -> array, as ``out_view`` gives them): views, no copy"""
    import torch
    from .models.gaussian_model import GaussianModel
    m = GaussianModel(device_name)
    m.sh_degree = sh_degree
    shapes = {"_features_dc": (1, 3), "_features_rest": (K, 3)}
    for attr, a in arrays.items():
        t = torch.as_tensor(a)[:n_out]
        setattr(m, attr, t.view((n_out,) + shapes[attr]) if attr in shapes else t)
    if K == 0:
        m._features_rest = torch.empty((n_out, 0, 3), dtype=torch.float32, device=m._xyz.device)
    return m


def call_tail(device, on):
    """-> the last three arguments of a stateless entry point, (on_device, device, stream), once torch's stream on the device has
    finished what produced the arrays"""
    if on:
        import torch
        torch.cuda.current_stream(device).synchronize()
    return 1 if on else 0, device, C.c_void_p(_m.stream_ptr(device, on))
