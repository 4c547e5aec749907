"""``mse`` / ``psnr`` / ``ssim`` with the names and definitions of the reference's ``src/utils/evaluation_utils.py`` on ``(1,3,H,W)``
(or ``(3,H,W)``) images.  CUDA tensors go through the fused metrics kernel (``gsr_image_metrics``: float64 sums, fixed order); host
tensors keep plain torch arithmetic -- they are small-image conveniences, not a fall-back of the device path."""
from __future__ import annotations

import math

import torch

from .. import raster


def _chw(img):
    if img.dim() == 4:
        if img.shape[0] != 1:
            raise NotImplementedError("the metrics take one image at a time: (1, 3, H, W)")
        img = img[0]
    return img


def _device_pair(img1, img2):
    """The two images as (3,H,W) float32 on one CUDA device, or None when neither is there."""
    if not (img1.is_cuda or img2.is_cuda):
        return None
    dev = img1.device if img1.is_cuda else img2.device
    return _chw(img1).to(dev, torch.float32), _chw(img2).to(dev, torch.float32)


def _window(window_size, sigma=1.5):
    """(k, k) float32: the outer product of the normalised 1-D Gaussian window"""
    offset = torch.arange(window_size, dtype=torch.float64) - window_size // 2
    g = torch.exp(-0.5 * (offset / sigma) ** 2).float()
    g = g / g.sum()
    return torch.outer(g, g)


def mse(img1, img2):
    pair = _device_pair(img1, img2)
    if pair is not None:
        return torch.tensor(raster.image_metrics(*pair)[0], dtype=torch.float32, device=pair[0].device)
    return ((img1 - img2) ** 2).mean()


def psnr(img1, img2):
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2)))


def ssim(img1, img2, window_size=11, size_average=True):
    if window_size != 11 or not size_average:
        raise NotImplementedError("ssim: only the 11 x 11 window with size_average=True is implemented (what the evaluation uses)")
    pair = _device_pair(img1, img2)
    if pair is not None:
        return torch.tensor(raster.image_metrics(*pair)[1], dtype=torch.float32, device=pair[0].device)
    a, b = _chw(img1)[None].float(), _chw(img2)[None].float()
    ch = a.shape[1]
    w = _window(window_size).expand(ch, 1, window_size, window_size).contiguous()
    conv = lambda x: torch.nn.functional.conv2d(x, w, padding=window_size // 2, groups=ch)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()


def metrics(img1, img2):
    """-> dict(mse, rmse, psnr, ssim) of Python floats from ONE kernel pass (CUDA tensors), what the evaluator logs per image."""
    pair = _device_pair(img1, img2)
    if pair is not None:
        m, s = raster.image_metrics(*pair)
    else:
        m, s = float(mse(img1, img2)), float(ssim(img1, img2))
    return {"mse": m, "rmse": math.sqrt(m), "psnr": 20.0 * math.log10(1.0 / math.sqrt(m)) if m > 0 else float("inf"), "ssim": s}
