"""Fine-tuning of a (merged) splat model against photographs through the differentiable rasteriser (``raster.render_differentiable``,
DESIGN.md 26): a short ``torch.optim.Adam`` run on the per-splat appearance -- DC colour, the other SH coefficients, opacity, optionally the
positions -- that removes what a colour transform per scene (``match_colors``) and the moment-matching of pairs (``fuse_overlap``) leave at a
seam.  The forward and backward passes are the HIP kernels of ``csrc/raster.hip``; the optimiser is plain torch, and so are the per-pixel
losses ``"l2"`` and ``"l1"``.  ``loss="l1_dssim"`` is the loss 3DGS scenes were trained with, ``(1 - lambda) L1 + lambda (1 - SSIM)`` with
``lambda_dssim = 0.2``: value and gradient come from one fused HIP kernel (``loss.l1_dssim``, ``csrc/imgloss.hip``) in
float64 with a fixed order of summation, so the promise below -- two runs give the same bits -- holds with it too.

The shape of the splats is tuned through ``"scaling"`` (log-scales) and ``"rotation"`` (raw quaternions), never through ``_covariance``
itself: the model keeps ``_scaling`` / ``_rotation`` beside ``_covariance`` and the ``.ply`` stores those two, so a tuned ``_covariance`` alone
could not be saved.  With either of the two in ``params`` every iteration builds ``cov6 = covariance_from_scale_rotation(scaling, rotation)``
(``covariance.py``, ``csrc/covgrad.hip``) in front of the rasteriser, and the run ends by writing back a triple that is consistent
bit for bit: ``_scaling``, ``_rotation`` (raw, not renormalised: the map ignores the quaternion's norm and its gradient is orthogonal to it)
and ``_covariance = build_covariance(_scaling, _rotation)``.  The run starts from the stored ``_scaling`` / ``_rotation`` when they reproduce
``_covariance`` (``FinetuneParams.geometry_rtol``), else from the exact decomposition of ``_covariance``; ``FinetuneResult.geometry_source`` says
which.  Without the two names nothing of this runs and the bits are those of the appearance-only tuner.

No densification, no clamp or regulariser on the scales, one camera per iteration.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from . import covariance
from . import loss as image_loss
from . import raster
from .utils.rasterization_util import _camera_args

TUNABLE = ("dc", "sh_rest", "opacity", "xyz", "scaling", "rotation")
GEOMETRY = ("scaling", "rotation")


@dataclass
class FinetuneParams:
    """The learning rates are those published with 3DGS (feature 2.5e-3, the other SH coefficients a twentieth of it, opacity 0.05, position
    1.6e-4, scaling 5e-3, rotation 1e-3).  ``params``: which tensors are tuned, of ``TUNABLE``.  ``loss``: ``"l2"`` (mean squared error),
    ``"l1"`` or ``"l1_dssim"`` (``(1 - lambda_dssim) L1 + lambda_dssim (1 - SSIM)``, the fused kernel of ``loss.l1_dssim``).
    ``geometry_rtol``: when ``"scaling"`` or ``"rotation"`` is tuned, the stored ``_scaling`` / ``_rotation`` are the starting point if the
    covariance built from them deviates from ``_covariance`` by at most this fraction of the row's Frobenius norm in every row.  A
    consistent triple rebuilt in float32 or carried through a rigid motion or a warp deviates by 1e-6 to 1e-5; the inconsistent states
    (no ``_scaling``, or ``from_mixture(decompose=True)``, whose "scaling" is the eigenvalue itself) are wrong by O(1)."""
    iterations: int = 200
    params: tuple = ("dc", "sh_rest", "opacity")
    lr_dc: float = 2.5e-3
    lr_sh_rest: float = 1.25e-4
    lr_opacity: float = 0.05
    lr_xyz: float = 1.6e-4
    loss: str = "l2"
    background: tuple = (0.0, 0.0, 0.0)
    # keyword-only: the positional order of the fields around them (``lambda_dssim`` last) is what it was
    lr_scaling: float = field(default=5e-3, kw_only=True)
    lr_rotation: float = field(default=1e-3, kw_only=True)
    geometry_rtol: float = field(default=1e-3, kw_only=True)
    lambda_dssim: float = 0.2


@dataclass
class FinetuneResult:
    losses: list = field(default_factory=list)              # one per iteration, the loss of the camera visited
    psnr_before: list = field(default_factory=list)         # per camera, in list order
    psnr_after: list = field(default_factory=list)
    iterations: int = 0
    error_list: list = field(default_factory=list)
    geometry_source: str = None                             # "stored" or "decomposed" when scaling / rotation is tuned, else None


def _psnr(image, target):
    mse, _ = raster.image_metrics(image.permute(2, 0, 1).contiguous(), target.permute(2, 0, 1).contiguous())
    return 20.0 * math.log10(1.0 / math.sqrt(mse)) if mse > 0 else math.inf


class ModelFinetuner:
    """``ModelFinetuner(model, cameras, images, params).run()`` -> ``FinetuneResult`` (``None`` when cancelled: the model is left alone).
    ``images``: one ``(H, W, 3)`` float32 image in [0, 1] per camera (arrays or tensors), or a directory holding
    ``<camera.image_name>.png``; a camera whose photograph is missing or of another size is skipped and named in ``error_list``.  Cameras are
    visited round-robin in list order and nothing draws random numbers: two runs give the same bits.  The tuned tensors are written back
    into ``model`` (which must be on a CUDA device)."""

    def __init__(self, model, cameras, images, params=None, device=None):
        self.model = model
        self.cameras = list(cameras)
        self.params = params if params is not None else FinetuneParams()
        unknown = [p for p in self.params.params if p not in TUNABLE]
        if unknown:
            raise ValueError(f"FinetuneParams.params: unknown tensor {unknown[0]!r} {TUNABLE} (the covariance is not tunable as a tensor of its own: "
                             "its shape is tuned through 'scaling' and 'rotation', DESIGN.md 31)")
        if not self.params.params:
            raise ValueError("FinetuneParams.params is empty")
        if self.params.loss not in ("l2", "l1", "l1_dssim"):
            raise ValueError(f"FinetuneParams.loss: {self.params.loss!r} (l2, l1, l1_dssim)")
        if self.params.loss == "l1_dssim" and not 0.0 <= float(self.params.lambda_dssim) <= 1.0:
            raise ValueError(f"FinetuneParams.lambda_dssim: {self.params.lambda_dssim!r} outside [0, 1]")
        self.images = images
        self.device = torch.device(device if device is not None else model.get_xyz.device)
        if self.device.type != "cuda":
            raise RuntimeError("ModelFinetuner needs the model on a CUDA device: the rasteriser has no CPU fallback")
        self.signal_cancel = False

    def cancel(self):
        self.signal_cancel = True

    def _targets(self, errors):
        """-> [(camera, target (H, W, 3) on the device)] of the cameras that have a photograph of their size"""
        pairs = []
        for k, cam in enumerate(self.cameras):
            if isinstance(self.images, (str, os.PathLike)):
                from .workers.evaluator import _read_image
                path = os.path.join(self.images, cam.image_name + ".png")
                try:
                    img = _read_image(path)[0].permute(1, 2, 0)
                except (OSError, IOError) as e:
                    errors.append(str(e))
                    continue
            else:
                img = self.images[k]
                img = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img, dtype=np.float32))
            img = img.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(img.shape) != (int(cam.height), int(cam.width), 3):
                errors.append(f"{cam.image_name}: image is {tuple(img.shape[:2])}, camera renders {(int(cam.height), int(cam.width))}")
                continue
            pairs.append((cam, img))
        return pairs

    def run(self):
        p, m, dev = self.params, self.model, self.device
        index = dev.index if dev.index is not None else 0
        result = FinetuneResult()
        pairs = self._targets(result.error_list)
        n = len(m)
        K = int(m._features_rest.shape[1]) if m._features_rest.numel() else 0
        tensors = {"xyz": m.get_xyz.detach().to(dev).reshape(n, 3), "dc": m._features_dc.detach().to(dev).reshape(n, 3),
                   "sh_rest": m._features_rest.detach().to(dev).reshape(n, K, 3) if K else None, "opacity": m._opacity.detach().to(dev).reshape(n)}
        cov6 = m.get_covariance().detach().to(dev).reshape(n, 6).contiguous()
        geometry = n > 0 and any(name in p.params for name in GEOMETRY)
        if geometry:
            tensors["scaling"], tensors["rotation"], result.geometry_source = self._geometry(cov6)
        else:
            tensors["scaling"] = tensors["rotation"] = None
        tuned = [name for name in TUNABLE if name in p.params and tensors[name] is not None and tensors[name].numel()]
        for name in tuned:
            tensors[name] = tensors[name].clone().contiguous().requires_grad_(True)
        lr = {"dc": p.lr_dc, "sh_rest": p.lr_sh_rest, "opacity": p.lr_opacity, "xyz": p.lr_xyz, "scaling": p.lr_scaling, "rotation": p.lr_rotation}

        def render(cam):
            # the shape is tuned through its factors: the covariance is rebuilt from them in front of every render (the one not tuned is a constant)
            cov = covariance.covariance_from_scale_rotation(tensors["scaling"], tensors["rotation"]) if geometry else cov6
            return raster.render_differentiable(tensors["xyz"], cov, tensors["opacity"], tensors["dc"], tensors["sh_rest"], m.sh_degree, *_camera_args(cam),
                                                background=p.background, radius_clip=3.0, device=index)[0]
        with torch.no_grad():
            result.psnr_before = [_psnr(render(cam), tgt) for cam, tgt in pairs]
        if pairs and tuned and n:
            opt = torch.optim.Adam([{"params": [tensors[name]], "lr": lr[name]} for name in tuned], eps=1e-15)
            for it in range(int(p.iterations)):
                if self.signal_cancel:
                    return None
                cam, tgt = pairs[it % len(pairs)]
                opt.zero_grad(set_to_none=True)
                if p.loss == "l1_dssim":
                    loss = image_loss.l1_dssim(render(cam), tgt, p.lambda_dssim)
                else:
                    diff = render(cam) - tgt
                    loss = (diff * diff).mean() if p.loss == "l2" else diff.abs().mean()
                loss.backward()
                opt.step()
                result.losses.append(float(loss.detach()))
                result.iterations = it + 1
        with torch.no_grad():
            result.psnr_after = [_psnr(render(cam), tgt) for cam, tgt in pairs]
        if "xyz" in tuned:
            m._xyz = tensors["xyz"].detach().reshape(m._xyz.shape).to(m._xyz.device)
        if "dc" in tuned:
            m._features_dc = tensors["dc"].detach().reshape(m._features_dc.shape).to(m._features_dc.device)
        if "sh_rest" in tuned:
            m._features_rest = tensors["sh_rest"].detach().reshape(m._features_rest.shape).to(m._features_rest.device)
        if "opacity" in tuned:
            m._opacity = tensors["opacity"].detach().reshape(m._opacity.shape).to(m._opacity.device)
        if geometry:                     # all three, consistent bit for bit: what save_ply stores rebuilds exactly what is rendered
            home = m._covariance.device
            m._scaling = tensors["scaling"].detach().reshape(n, 3).to(home)
            m._rotation = tensors["rotation"].detach().reshape(n, 4).to(home)
            m._covariance = torch.as_tensor(covariance.build_covariance(tensors["scaling"].detach(), tensors["rotation"].detach())).reshape(n, 6).to(home)
        return result

    def _geometry(self, cov6):
        """-> (scaling (n, 3), rotation (n, 4), "stored" | "decomposed") on the device: the model's ``_scaling`` / ``_rotation`` when the covariance
        built from them reproduces ``cov6`` row by row within ``geometry_rtol`` of the row's Frobenius norm, else ``GSR_DECOMP_EXACT`` of ``cov6``
        (log standard deviations, unit quaternion)"""
        m, dev, n = self.model, self.device, int(cov6.shape[0])
        if tuple(m._scaling.shape) == (n, 3) and tuple(m._rotation.shape) == (n, 4):
            scaling = m._scaling.detach().to(device=dev, dtype=torch.float32).contiguous()
            rotation = m._rotation.detach().to(device=dev, dtype=torch.float32).contiguous()
            built = torch.as_tensor(covariance.build_covariance(scaling, rotation))
            twice = built.new_tensor([1.0, 2.0, 2.0, 1.0, 2.0, 1.0])              # an off-diagonal entry stands for two of the nine
            frob = lambda c: torch.sqrt((c.double() ** 2 * twice.double()).sum(dim=1))
            if bool((frob(built - cov6) <= float(self.params.geometry_rtol) * frob(cov6)).all()):          # (a NaN row fails the comparison)
                return scaling, rotation, "stored"
        scaling, rotation, _ = m._decompose(_lib.GSR_DECOMP_EXACT)
        return scaling.to(dev).contiguous(), rotation.to(dev).contiguous(), "decomposed"
