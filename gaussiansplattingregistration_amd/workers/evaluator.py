"""Headless ``RegistrationEvaluator`` (reference ``src/gui/workers/graphics/qt_evaluator.py:16-155``): merge the two clouds with the
registration result, render the merged model from every training camera and compare with the photographs.  Same constructor,
same JSON log (``registration_data``, ``mse``, ``rmse``, ``ssim``, ``psnr``, ``lpips``, ``error_list``); no Qt.

LPIPS needs the pretrained AlexNet weights the ``lpips`` package downloads; they are not part of this backend, so ``lpips`` is
``null`` in the log and ``error_list`` says why.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from ..models.gaussian_model import GaussianModel
from ..utils.evaluation_utils import metrics
from ..utils.rasterization_util import rasterize_image

LPIPS_NOTE = "lpips: not computed (the pretrained LPIPS network weights are not available to this backend)"


def _read_image(path):
    """``(1, 3, H, W)`` float32 in [0, 1] of an image file, as ``to_tensor(Image.open(path).convert('RGB'))`` gives it."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1)[None].contiguous()


LOG_FIELDS = ("registration_data", "mse", "rmse", "ssim", "psnr", "lpips", "error_list")       # the reference's log, in its order


def _json_value(v):
    """what goes into the log: arrays as nested lists, numbers that JSON cannot carry (nan, +-inf) as null"""
    if isinstance(v, (np.ndarray, torch.Tensor)):
        v = v.tolist()
    if isinstance(v, dict):
        return {str(k): _json_value(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_value(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return float(v) if math.isfinite(v) else None
    if isinstance(v, np.integer):
        return int(v)
    return v


@dataclass
class EvaluationObject:
    """One evaluation: the registration record it belongs to (its fields, or empty) and the means over the images."""
    registration_data: dict = field(default_factory=dict)
    mse: float = None
    rmse: float = None
    ssim: float = None
    psnr: float = None
    lpips: float = None
    error_list: list = field(default_factory=list)

    def to_json(self):
        return {k: _json_value(getattr(self, k)) for k in LOG_FIELDS}


class RegistrationEvaluator:
    EvaluationObject = EvaluationObject

    def __init__(self, pc1, pc2, transformation, cameras_list, images_path, log_path, color, registration_result, use_gpu, rotate_sh=False, with_scaling=False,
                 fuse=None, match_colors=None, match_colors_gate=None):
        self.signal_cancel = False
        self.pc1 = pc1
        self.pc2 = pc2
        self.transformation = transformation
        self.cameras_list = cameras_list
        self.images_path = images_path
        self.log_path = log_path
        self.color = color
        self.use_gpu = use_gpu              # whether the metrics run on the device; the rasteriser always does
        self.device = "cuda:0"
        self.rotate_sh = rotate_sh
        self.with_scaling = bool(with_scaling)          # the transformation is a similarity [c R | t]: merged through gsr_model_similarity
        self.fuse = fuse                    # FuseOverlapParams or None: the merge stores the splats the two clouds share once (fuse_overlap)
        self.match_colors, self.match_colors_gate = match_colors, match_colors_gate      # ColorMatchParams or None: colours harmonised before the merge
        self.registration_result = registration_result
        self.mean_mses = self.mean_rmses = self.mean_ssims = self.mean_psnrs = self.mean_lpipss = None
        self.per_image = []
        self.current_progress = 0
        self.max_progress = len(cameras_list)
        self.on_render = None               # optional callback(camera, image (1,H,W,3)): scripts/evaluate_registration.py --save-renders

    def cancel_evaluation(self):
        self.signal_cancel = True

    def run(self):
        """-> the ``EvaluationObject`` written to ``log_path``, or ``None`` when cancelled (polled between cameras)."""
        point_cloud = None                  # merged and moved to the device when the first photograph has been read
        error_list = []
        rows = []
        for camera in self.cameras_list:
            if self.signal_cancel:
                return None
            self.current_progress += 1
            image_path = os.path.join(self.images_path, camera.image_name + ".png")
            try:
                gt_image = _read_image(image_path)
                if self.use_gpu:
                    gt_image = gt_image.to(self.device)
            except (OSError, IOError) as e:
                error_list.append(str(e))
                continue
            if point_cloud is None:
                point_cloud = GaussianModel.get_merged_gaussian_point_clouds(self.pc1, self.pc2, self.transformation, rotate_sh=self.rotate_sh,
                                                                             with_scaling=self.with_scaling, fuse=self.fuse, match_colors=self.match_colors,
                                                                             match_colors_gate=self.match_colors_gate)
                point_cloud.move_to_device(self.device)
            render = rasterize_image(point_cloud, camera, 1, self.color, self.device, self.use_gpu)
            if self.on_render is not None:
                self.on_render(camera, render)
            image_tensor = render.permute(0, 3, 1, 2)
            if tuple(image_tensor.shape) != tuple(gt_image.shape):
                error_list.append(f"{image_path}: image is {tuple(gt_image.shape[2:])}, camera renders {tuple(image_tensor.shape[2:])}")
                continue
            rows.append(dict(metrics(image_tensor, gt_image), image_name=camera.image_name))
        self.per_image = rows
        mean = lambda k: float(np.mean([r[k] for r in rows])) if rows else None          # no image compared: null in the log
        self.mean_mses, self.mean_rmses, self.mean_ssims, self.mean_psnrs = mean("mse"), mean("rmse"), mean("ssim"), mean("psnr")
        self.mean_lpipss = None
        error_list.append(LPIPS_NOTE)
        return self.create_and_save_log_file(error_list)

    def create_and_save_log_file(self, error_list):
        record = vars(self.registration_result) if self.registration_result is not None else {}
        evaluation = EvaluationObject(dict(record), self.mean_mses, self.mean_rmses, self.mean_ssims, self.mean_psnrs, self.mean_lpipss, list(error_list))
        with open(self.log_path, "w") as out:
            json.dump(evaluation.to_json(), out, indent=2, allow_nan=False)
        return evaluation
