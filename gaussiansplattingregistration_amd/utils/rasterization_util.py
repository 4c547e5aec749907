"""``rasterize_image`` with the signature of the reference's ``src/utils/rasterization_util.py:10-31``.  The reference hands the
model to gsplat's CUDA rasteriser; here the image comes from this project's HIP rasteriser (``csrc/raster.hip``), which restates
the same published forward pass.  gsplat does not exist on ROCm, so parity with it is unpinned."""
from __future__ import annotations

import torch

from .. import raster


def rasterize_image(point_cloud, camera, scale, color, device, leave_on_gpu=True):
    """-> ``(1, H, W, 3)`` float32: the model seen from ``camera`` over the background ``color``; covariances are
    ``point_cloud.get_full_covariance(scale)``, SH up to the model's degree, splats of 3 px radius or less dropped."""
    dev = torch.device(device)
    index = dev.index if dev.index is not None else 0
    K = camera.intrinsics[0]
    image = raster.render_model(point_cloud, camera.viewmat[0], float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), int(camera.width),
                                int(camera.height), background=color, scale=scale, radius_clip=3.0, device=index)[None]
    return image if leave_on_gpu else image.cpu()


def _camera_args(camera):
    K = camera.intrinsics[0]
    return camera.viewmat[0], float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), int(camera.width), int(camera.height)


def rasterize_depth(point_cloud, camera, scale, device, leave_on_gpu=True, radius_clip=3.0):
    """-> ``(depth, alpha)``, two ``(H, W)`` float32 maps of the model seen from ``camera``: the expected depth
    ``sum z_i w_i / max(alpha, 1e-10)`` (camera-space z, blending weights of the RGB render; 0 where no splat counts) and the
    coverage ``alpha = 1 - T``.  The same culling as ``rasterize_image``; the reference has no such output."""
    dev = torch.device(device)
    index = dev.index if dev.index is not None else 0
    out = raster.render_model_aux(point_cloud, *_camera_args(camera), scale=scale, radius_clip=radius_clip, device=index, outputs=("depth", "alpha"))
    depth, alpha = out["depth"], out["alpha"]
    return (depth, alpha) if leave_on_gpu else (depth.cpu(), alpha.cpu())
