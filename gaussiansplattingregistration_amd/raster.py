"""ctypes front of the splat rasteriser and the image metrics (``csrc/raster.hip``; ``gsr_raster_*``, ``gsr_image_metrics``).

``RasterContext`` owns the library's grow-only workspaces; ``render`` (RGB) and ``render_aux`` (RGB, expected depth, coverage and the
per-splat largest blending weight) take the SoA arrays ``GaussianModel`` holds, as CUDA tensors
(zero-copy) or as host arrays (uploaded through torch first: the library's render entry takes device pointers only).  No GPU:
``RuntimeError`` -- there is no CPU fallback.

``render_backward`` is the backward pass of ``render_aux`` (``gsr_raster_backward``) and ``render_differentiable`` the
``torch.autograd.Function`` over the two: image and coverage with gradients for positions, covariances, opacities and SH coefficients.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import _marshal as _m


BACKWARD_OUTPUTS = ("xyz", "cov6", "raw_opacity", "dc", "sh_rest")


class RasterContext:
    def __init__(self, device: int = 0):
        self._L = _lib.load(require_device=True)
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.check(self._L.gsr_raster_create(C.byref(self._h), self.device, None), "gsr_raster_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.gsr_raster_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _inputs(self, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, background):
        """what both render entries take: the device, n, K, the five arrays as contiguous float32 CUDA tensors, viewmat and background as C arrays"""
        dev = torch.device("cuda", self.device)

        def up(a, shape):
            t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
            return t.detach().to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
        n = int(xyz.shape[0])
        K = 0 if sh_rest is None else int(np.prod(tuple(sh_rest.shape)[1:])) // 3
        arrays = (up(xyz, (n, 3)), up(cov6, (n, 6)), up(raw_opacity, (n,)), up(dc, (n, 3)), up(sh_rest, (n, 3 * K)) if K else None)
        V = (C.c_float * 16)(*np.asarray(viewmat.detach().cpu() if isinstance(viewmat, torch.Tensor) else viewmat, dtype=np.float32).reshape(16))
        bg = (C.c_float * 3)(*np.asarray(background, dtype=np.float32).reshape(3))
        return dev, n, K, arrays, V, bg

    def render(self, xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, viewmat, fx, fy, cx, cy, width, height, background=(0.0, 0.0, 0.0),
               radius_clip=3.0, with_stats=False):
        """-> image ``(H, W, 3)`` float32 CUDA tensor [, stats int64 CUDA tensor (visible splats, intersections, non-empty tiles)].
        ``sh_rest`` is ``(n, K, 3)`` (or ``(n, 3K)`` coefficient-major); ``viewmat`` the 4x4 world -> camera matrix."""
        dev, n, K, (t_xyz, t_cov, t_op, t_dc, t_sh), V, bg = self._inputs(xyz, cov6, raw_opacity, dc, sh_rest, viewmat, background)
        sh_degree = int(sh_degree)
        image = torch.empty((int(height), int(width), 3), dtype=torch.float32, device=dev)
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._L.gsr_raster_render(self._h, n, K, sh_degree, t_xyz.data_ptr(), t_cov.data_ptr(), t_op.data_ptr(), t_dc.data_ptr(),
                                             t_sh.data_ptr() if K else None, V, float(fx), float(fy), float(cx), float(cy), int(width), int(height), bg,
                                             float(radius_clip), image.data_ptr(), stats.data_ptr(), C.c_void_p(stream)), "gsr_raster_render")
        self._keep = (t_xyz, t_cov, t_op, t_dc, t_sh)         # alive until the next render: the blend is still enqueued
        return (image, stats) if with_stats else image

    def render_aux(self, xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, viewmat, fx, fy, cx, cy, width, height, background=(0.0, 0.0, 0.0),
                   radius_clip=3.0, outputs=("image", "depth", "alpha"), contribution=None, with_stats=False):
        """-> dict of float32 CUDA tensors, one per name in ``outputs``: ``image`` ``(H, W, 3)`` (the bits ``render`` gives), ``depth``
        ``(H, W)`` (expected depth ``sum z w / max(alpha, 1e-10)``, 0 where nothing counted), ``alpha`` ``(H, W)`` (``1 - T``); with
        ``with_stats`` also ``stats``.  ``contribution``: a contiguous float32 CUDA tensor of ``n``, raised IN PLACE to
        ``max(its value, the largest blending weight alpha T of each splat on this image)`` and returned under ``contribution`` -- it
        is not cleared, so one buffer collects the maximum over several cameras.  ``outputs`` may be empty when it is given."""
        outputs = tuple(outputs)
        unknown = [o for o in outputs if o not in ("image", "depth", "alpha")]
        if unknown:
            raise ValueError(f"render_aux: unknown output {unknown[0]!r} (image, depth, alpha)")
        dev, n, K, (t_xyz, t_cov, t_op, t_dc, t_sh), V, bg = self._inputs(xyz, cov6, raw_opacity, dc, sh_rest, viewmat, background)
        if contribution is not None:
            if not (isinstance(contribution, torch.Tensor) and contribution.is_cuda and contribution.device == dev and contribution.dtype == torch.float32
                    and contribution.is_contiguous() and contribution.numel() == n):
                raise ValueError(f"render_aux: contribution must be a contiguous float32 tensor of {n} elements on {dev}")
        if n == 0 and not outputs and contribution is not None:          # nothing to raise (an empty tensor's pointer is NULL: the library would see no output)
            return {"contribution": contribution, **({"stats": torch.zeros(3, dtype=torch.int64, device=dev)} if with_stats else {})}
        sh_degree = int(sh_degree)
        H, W = int(height), int(width)
        out = {}
        if "image" in outputs:
            out["image"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        for name in ("depth", "alpha"):
            if name in outputs:
                out[name] = torch.empty((H, W), dtype=torch.float32, device=dev)
        ptr = lambda name: out[name].data_ptr() if name in out else None
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self._L.gsr_raster_render_aux(self._h, n, K, sh_degree, t_xyz.data_ptr(), t_cov.data_ptr(), t_op.data_ptr(), t_dc.data_ptr(),
                                                 t_sh.data_ptr() if K else None, V, float(fx), float(fy), float(cx), float(cy), W, H, bg, float(radius_clip),
                                                 ptr("image"), ptr("depth"), ptr("alpha"), contribution.data_ptr() if contribution is not None else None, stats.data_ptr(),
                                                 C.c_void_p(stream)),
                   "gsr_raster_render_aux")
        self._keep = (t_xyz, t_cov, t_op, t_dc, t_sh)         # alive until the next render: the blend is still enqueued
        if contribution is not None:
            out["contribution"] = contribution
        if with_stats:
            out["stats"] = stats
        return out

    def render_backward(self, xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, viewmat, fx, fy, cx, cy, width, height, grad_image=None, grad_alpha=None,
                        background=(0.0, 0.0, 0.0), radius_clip=3.0, wants=BACKWARD_OUTPUTS, with_stats=False):
        """The backward pass of ``render_aux`` -> dict of float32 CUDA tensors, one per name in ``wants``: ``xyz`` ``(n, 3)``,
        ``cov6`` ``(n, 6)``, ``raw_opacity`` ``(n,)``, ``dc`` ``(n, 3)``, ``sh_rest`` ``(n, 3K)`` (coefficient-major, as ``render`` takes it), the
        gradients of a loss whose derivatives with respect to the image ``(H, W, 3)`` and the coverage ``(H, W)`` are ``grad_image`` and
        ``grad_alpha`` (either may be None, not both; host arrays are uploaded).  Culled splats get exact zeros.  The call renders
        nothing and relies on no earlier render; with ``with_stats`` also ``stats``."""
        wants = tuple(wants)
        unknown = [o for o in wants if o not in BACKWARD_OUTPUTS]
        if unknown:
            raise ValueError(f"render_backward: unknown output {unknown[0]!r} {BACKWARD_OUTPUTS}")
        if not wants:
            raise ValueError("render_backward: no output requested")
        if grad_image is None and grad_alpha is None:
            raise ValueError("render_backward: grad_image and grad_alpha are both None")
        dev, n, K, (t_xyz, t_cov, t_op, t_dc, t_sh), V, bg = self._inputs(xyz, cov6, raw_opacity, dc, sh_rest, viewmat, background)
        H, W = int(height), int(width)

        def up(a, shape):
            if a is None:
                return None
            t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
            if tuple(t.shape) != shape:
                raise ValueError(f"render_backward: a gradient of shape {tuple(t.shape)}, expected {shape}")
            return t.detach().to(device=dev, dtype=torch.float32).contiguous()
        g_img, g_alpha = up(grad_image, (H, W, 3)), up(grad_alpha, (H, W))
        shapes = {"xyz": (n, 3), "cov6": (n, 6), "raw_opacity": (n,), "dc": (n, 3), "sh_rest": (n, 3 * K)}
        out = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in wants}
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
        if n > 0 and any(t.numel() for t in out.values()):               # (an empty tensor's pointer is NULL: the library would see no output)
            ptr = lambda name: out[name].data_ptr() if name in out and out[name].numel() else None
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self._L.gsr_raster_backward(self._h, n, K, int(sh_degree), t_xyz.data_ptr(), t_cov.data_ptr(), t_op.data_ptr(), t_dc.data_ptr(),
                                                   t_sh.data_ptr() if K else None, V, float(fx), float(fy), float(cx), float(cy), W, H, bg, float(radius_clip),
                                                   g_img.data_ptr() if g_img is not None else None, g_alpha.data_ptr() if g_alpha is not None else None,
                                                   ptr("xyz"), ptr("cov6"), ptr("raw_opacity"), ptr("dc"), ptr("sh_rest"), stats.data_ptr(), C.c_void_p(stream)),
                       "gsr_raster_backward")
            self._keep = (t_xyz, t_cov, t_op, t_dc, t_sh, g_img, g_alpha)         # alive until the next call: the kernels are still enqueued
        if with_stats:
            out["stats"] = stats
        return out

    def backward_timing(self):
        """-> {"preprocess", "sort", "blend_backward", "splat_backward"} milliseconds of the last ``render_backward`` (device events; waits for it)."""
        ms = (C.c_float * 4)()
        _lib.check(self._L.gsr_raster_get_backward_timing(self._h, ms), "gsr_raster_get_backward_timing")
        return {"preprocess": float(ms[0]), "sort": float(ms[1]), "blend_backward": float(ms[2]), "splat_backward": float(ms[3])}

    def timing(self):
        """-> {"preprocess", "sort", "blend"} milliseconds of the last render (device events; waits for it)."""
        ms = (C.c_float * 3)()
        _lib.check(self._L.gsr_raster_get_timing(self._h, ms), "gsr_raster_get_timing")
        return {"preprocess": float(ms[0]), "sort": float(ms[1]), "blend": float(ms[2])}


_contexts = {}


def context(device: int = 0) -> RasterContext:
    """The process-wide context of a device (workspaces are reused from image to image)."""
    if device not in _contexts:
        _contexts[device] = RasterContext(device)
    return _contexts[device]


class _RenderFunction(torch.autograd.Function):
    """``render_aux`` forwards, ``render_backward`` backwards.  Neither holds state in the shared context between the two calls."""

    @staticmethod
    def forward(ctx, xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, camera, background, radius_clip, device):
        viewmat, fx, fy, cx, cy, width, height = camera
        out = context(device).render_aux(xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, viewmat, fx, fy, cx, cy, width, height, background, radius_clip,
                                         outputs=("image", "alpha"))
        ctx.save_for_backward(xyz, cov6, raw_opacity, dc, sh_rest)
        ctx.call = (sh_degree, camera, background, radius_clip, device)
        return out["image"], out["alpha"]

    @staticmethod
    def backward(ctx, grad_image, grad_alpha):
        xyz, cov6, raw_opacity, dc, sh_rest = ctx.saved_tensors
        sh_degree, (viewmat, fx, fy, cx, cy, width, height), background, radius_clip, device = ctx.call
        wants = tuple(name for name, need in zip(BACKWARD_OUTPUTS, ctx.needs_input_grad[:5]) if need and not (name == "sh_rest" and sh_rest is None))
        if not wants:
            return (None,) * 10
        got = context(device).render_backward(xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, viewmat, fx, fy, cx, cy, width, height, grad_image, grad_alpha,
                                              background, radius_clip, wants)
        shapes = {"xyz": xyz, "cov6": cov6, "raw_opacity": raw_opacity, "dc": dc, "sh_rest": sh_rest}
        grads = tuple(got[name].reshape(shapes[name].shape).to(shapes[name].dtype) if name in got else None for name in BACKWARD_OUTPUTS)
        return grads + (None,) * 5


def render_differentiable(xyz, cov6, raw_opacity, dc, sh_rest, sh_degree, viewmat, fx, fy, cx, cy, width, height, background=(0.0, 0.0, 0.0),
                          radius_clip=3.0, device=0):
    """-> ``(image (H, W, 3), alpha (H, W))``, the bits ``render_aux`` gives, differentiable with respect to the five model tensors (CUDA
    tensors on ``device``; ``sh_rest`` ``(n, K, 3)``, ``(n, 3K)`` or None).  The camera arguments are not differentiable: pose gradients come
    from composing the motion in torch in front of this call (``xyz' = R xyz + t``, ``Sigma' = R Sigma R^T``).  Expected depth has no
    gradient and is not returned."""
    camera = (viewmat.detach() if isinstance(viewmat, torch.Tensor) else viewmat, float(fx), float(fy), float(cx), float(cy), int(width), int(height))
    return _RenderFunction.apply(xyz, cov6, raw_opacity, dc, sh_rest, int(sh_degree), camera, tuple(float(b) for b in background), float(radius_clip), int(device))


def render_model(model, viewmat, fx, fy, cx, cy, width, height, background=(0.0, 0.0, 0.0), scale=1.0, radius_clip=3.0, device=0, with_stats=False):
    """One image of a ``GaussianModel`` (its covariances times ``scale``^2, as ``get_full_covariance(scale)`` gives them)."""
    full = model.get_full_covariance(scale)
    cov6 = torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], dim=1)
    return context(device).render(model.get_xyz, cov6, model.get_raw_opacity, model.get_colors, model._features_rest, model.sh_degree, viewmat, fx, fy,
                                  cx, cy, width, height, background, radius_clip, with_stats)


def model_cov6(model, scale=1.0):
    """the six covariance terms the render entries take, of ``model.get_full_covariance(scale)``"""
    full = model.get_full_covariance(scale)
    return torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], dim=1)


def render_model_aux(model, viewmat, fx, fy, cx, cy, width, height, background=(0.0, 0.0, 0.0), scale=1.0, radius_clip=3.0, device=0,
                     outputs=("image", "depth", "alpha"), contribution=None, with_stats=False):
    """``RasterContext.render_aux`` of a ``GaussianModel`` (its covariances times ``scale``^2)."""
    return context(device).render_aux(model.get_xyz, model_cov6(model, scale), model.get_raw_opacity, model.get_colors, model._features_rest, model.sh_degree, viewmat, fx, fy,
                                      cx, cy, width, height, background, radius_clip, outputs, contribution, with_stats)


def image_metrics(a, b, device=None):
    """-> (mse, ssim) as Python floats (the kernel's float64 sums) of two ``(3, H, W)`` float32 images, host arrays or CUDA tensors."""
    L = _lib.load(require_device=True)
    if tuple(a.shape) != tuple(b.shape) or len(a.shape) != 3 or a.shape[0] != 3:
        raise ValueError(f"image_metrics takes two (3, H, W) images, got {tuple(a.shape)} and {tuple(b.shape)}")
    _, H, W = (int(s) for s in a.shape)
    if device is None:
        device = a.device.index if _m.is_cuda(a) else b.device.index if _m.is_cuda(b) else 0
    if _m.is_cuda(a) != _m.is_cuda(b):             # one side on the device: bring the other there
        dev = torch.device("cuda", device)
        a, b = (torch.as_tensor(np.asarray(t, dtype=np.float32)).to(dev) if not _m.is_cuda(t) else t for t in (a, b))
    pa, ka, on = _m.prep(a, (3, H, W), np.float32, device)
    pb, kb, _ = _m.prep(b, (3, H, W), np.float32, device)
    out = (C.c_double * 2)()
    _lib.check(L.gsr_image_metrics(pa, pb, H, W, 1 if on else 0, out, device, C.c_void_p(_m.stream_ptr(device, on))), "gsr_image_metrics")
    return float(out[0]), float(out[1])
