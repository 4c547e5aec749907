"""ctypes front of the fine-tuner's photometric loss (``csrc/imgloss.hip``; ``gsr_loss_*``):
``(1 - lambda) L1 + lambda (1 - SSIM)`` of an ``(H, W, 3)`` image against a target and its gradient with respect to the image, one fused
HIP kernel in float64 with a fixed order of summation -- the same inputs give the same bits.  The SSIM is the one ``raster.image_metrics``
reports.  ``LossContext`` owns the library's grow-only buffer of tile partials; ``l1_dssim`` is the ``torch.autograd.Function`` over it.
No GPU, or tensors on the host: ``RuntimeError`` -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


class LossContext:
    def __init__(self, device: int = 0):
        self._L = _lib.load(require_device=True)
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.check(self._L.gsr_loss_create(self.device, C.byref(self._h)), "gsr_loss_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.gsr_loss_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def l1_dssim(self, image, target, lambda_dssim=0.2, with_grad=True, parts_out=None, grad_out=None):
        """-> ``(parts, grad)``: ``parts`` a float64 tensor ``(loss, l1, ssim)`` on the device, ``grad`` the ``(H, W, 3)`` float32 gradient with
        respect to ``image`` (None without ``with_grad``: the adjoint half of the kernel is skipped, ``parts`` has the same bits).  Enqueued
        on torch's current stream; nothing waits.  ``parts_out`` / ``grad_out``: tensors to overwrite instead of new ones."""
        dev = torch.device("cuda", self.device)
        for name, t in (("image", image), ("target", target)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise RuntimeError(f"l1_dssim: {name} is not a CUDA tensor (the loss kernel has no CPU fallback)")
            if t.device != dev:
                raise RuntimeError(f"l1_dssim: {name} lives on {t.device}, the context on {dev}")
        if image.dim() != 3 or image.shape[2] != 3 or tuple(image.shape) != tuple(target.shape):
            raise ValueError(f"l1_dssim takes two (H, W, 3) images, got {tuple(image.shape)} and {tuple(target.shape)}")
        H, W = int(image.shape[0]), int(image.shape[1])
        a = image.detach().to(torch.float32).contiguous()
        b = target.detach().to(torch.float32).contiguous()
        parts = parts_out if parts_out is not None else torch.empty(3, dtype=torch.float64, device=dev)
        grad = None
        if with_grad:
            grad = grad_out if grad_out is not None else torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._L.gsr_loss_l1_dssim(self._h, a.data_ptr(), b.data_ptr(), H, W, float(lambda_dssim), parts.data_ptr(),
                                             grad.data_ptr() if grad is not None else None, C.c_void_p(stream)), "gsr_loss_l1_dssim")
        return parts, grad


_contexts = {}


def context(device: int = 0) -> LossContext:
    """The process-wide context of a device (its buffer is reused from image to image)."""
    if device not in _contexts:
        _contexts[device] = LossContext(device)
    return _contexts[device]


class _L1DssimFunction(torch.autograd.Function):
    """The kernel forwards, with the gradient when the image wants one; backwards the stored gradient times the incoming scalar."""

    @staticmethod
    def forward(ctx, image, target, lambda_dssim):
        parts, grad = context(image.device.index).l1_dssim(image, target, lambda_dssim, with_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        ctx.like = (image.shape, image.dtype)
        ctx.mark_non_differentiable(parts)
        return parts[0].to(torch.float32), parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        grad, = ctx.saved_tensors
        if grad is None or not ctx.needs_input_grad[0]:
            return None, None, None
        shape, dtype = ctx.like
        return (grad * grad_loss).reshape(shape).to(dtype), None, None


def l1_dssim(image, target, lambda_dssim=0.2, return_parts=False):
    """-> the scalar float32 loss ``(1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM)`` of two ``(H, W, 3)`` CUDA tensors, differentiable with
    respect to ``image`` (the target gets no gradient).  ``return_parts``: ``(loss, parts)`` with ``parts`` the kernel's float64
    ``(loss, l1, ssim)`` on the device, from the same launch."""
    for name, t in (("image", image), ("target", target)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"loss.l1_dssim: {name} is not a CUDA tensor (the loss kernel has no CPU fallback)")
    if not 0.0 <= float(lambda_dssim) <= 1.0:
        raise ValueError(f"loss.l1_dssim: lambda_dssim {lambda_dssim!r} outside [0, 1]")
    loss, parts = _L1DssimFunction.apply(image, target, float(lambda_dssim))
    return (loss, parts) if return_parts else loss
