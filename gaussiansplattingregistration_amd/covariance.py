"""Covariance of a splat from its log-scales and raw quaternion, and the derivative of that map (``csrc/covgrad.hip``):
``cov = R(q / |q|) diag(exp(s))^2 R^T``, the float32 arithmetic the ``.ply`` loader runs (``gsr_ply_unpack``), so a covariance rebuilt here
from a loaded model's ``_scaling`` / ``_rotation`` has the bits of its ``_covariance``.

``build_covariance`` and ``build_covariance_backward`` are the two kernels; ``covariance_from_scale_rotation`` is the ``torch.autograd``
node over them that the fine-tuner puts in front of ``raster.render_differentiable`` to tune the shape of the splats.  CUDA tensors are
used where they lie and the results are CUDA tensors; host arrays are uploaded by the library and the results are numpy arrays.  No GPU:
``RuntimeError`` -- there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import _marshal as _m
from . import _model_view as _mv

BACKWARD_OUTPUTS = ("scaling", "rotation")


def _rows(a):
    return int(a.shape[0]) if hasattr(a, "shape") else len(a)


def _inputs(arrays, shapes, device):
    """-> (pointers, keep-alives, on_device, device) of arrays that are all CUDA tensors of one device or all on the host"""
    if device is None:
        device = next((a.device.index for a in arrays if _m.is_cuda(a)), 0)
    prepared = [_m.prep(a, shape, np.float32, device) for a, shape in zip(arrays, shapes)]
    on = [p[2] for p in prepared]
    if any(o != on[0] for o in on):
        raise RuntimeError("the arrays must all be CUDA tensors of one device or all live on the host")
    return [p[0] for p in prepared], [p[1] for p in prepared], on[0], device


def build_covariance(scaling, rotation, device=None):
    """``scaling`` ``(n, 3)`` log-scales, ``rotation`` ``(n, 4)`` raw quaternions ``(w, x, y, z)`` -> ``cov6`` ``(n, 6)`` float32
    ``(xx, xy, xz, yy, yz, zz)``: ``gsr_cov_build``.  A row with ``|q| = 0`` or a non-finite entry comes back as NaN, as from the loader."""
    L = _lib.load(require_device=True)
    n = _rows(scaling)
    (ps, pq), keep, on, device = _inputs((scaling, rotation), ((n, 3), (n, 4)), device)
    cov, pc = _m.out((n, 6), np.float32, device, on)
    _lib.check(L.gsr_cov_build(ps, pq, n, pc, *_mv.call_tail(device, on)), "gsr_cov_build")
    return cov


def build_covariance_backward(scaling, rotation, grad_cov6, wants=BACKWARD_OUTPUTS, device=None):
    """``grad_cov6`` ``(n, 6)`` = dLoss/dcov6 as ``render_backward`` returns it (an off-diagonal entry stands for both symmetric positions)
    -> dict with ``scaling`` ``(n, 3)`` and ``rotation`` ``(n, 4)``, or the one of them named in ``wants``: ``gsr_cov_build_backward``.  A row whose
    ``grad_cov6`` is all zero gets exact zeros; the gradient of the quaternion is orthogonal to it and scales with ``1 / |q|``."""
    wants = tuple(wants)
    unknown = [o for o in wants if o not in BACKWARD_OUTPUTS]
    if unknown:
        raise ValueError(f"build_covariance_backward: unknown output {unknown[0]!r} {BACKWARD_OUTPUTS}")
    if not wants:
        raise ValueError("build_covariance_backward: no output requested")
    L = _lib.load(require_device=True)
    n = _rows(scaling)
    (ps, pq, pg), keep, on, device = _inputs((scaling, rotation, grad_cov6), ((n, 3), (n, 4), (n, 6)), device)
    shapes = {"scaling": (n, 3), "rotation": (n, 4)}
    got = {name: _m.out(shapes[name], np.float32, device, on) for name in wants}
    ptr = lambda name: got[name][1] if name in got else None
    if n > 0:                                                    # (an empty tensor's pointer is NULL: the library would see no output)
        _lib.check(L.gsr_cov_build_backward(ps, pq, pg, n, ptr("scaling"), ptr("rotation"), *_mv.call_tail(device, on)), "gsr_cov_build_backward")
    return {name: o for name, (o, _) in got.items()}


class _CovarianceFunction(torch.autograd.Function):
    """``gsr_cov_build`` forwards, ``gsr_cov_build_backward`` backwards; the backward recomputes what it needs from the two inputs."""

    @staticmethod
    def forward(ctx, scaling, rotation):
        ctx.save_for_backward(scaling, rotation)
        return torch.as_tensor(build_covariance(scaling.detach(), rotation.detach()))

    @staticmethod
    def backward(ctx, grad_cov6):
        scaling, rotation = ctx.saved_tensors
        wants = tuple(name for name, need in zip(BACKWARD_OUTPUTS, ctx.needs_input_grad) if need)
        if not wants:
            return None, None
        got = build_covariance_backward(scaling.detach(), rotation.detach(), grad_cov6.detach().to(scaling.device), wants)
        like = {"scaling": scaling, "rotation": rotation}
        return tuple(torch.as_tensor(got[name]).reshape(like[name].shape).to(like[name].dtype) if name in got else None for name in BACKWARD_OUTPUTS)


def covariance_from_scale_rotation(scaling, rotation):
    """-> ``cov6`` ``(n, 6)``, the bits of ``build_covariance``, differentiable with respect to both tensors (``(n, 3)`` and ``(n, 4)``, on one
    device).  The backward pass asks the kernel only for the inputs that need a gradient."""
    return _CovarianceFunction.apply(scaling, rotation)
