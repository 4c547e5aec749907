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
from ..utils.rasterization_util import rasterize_depth, rasterize_image

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
                 fuse=None, match_colors=None, match_colors_gate=None, warp=None):
        self.signal_cancel = False
        self.warp = warp                    # warp.WarpField or None: the first cloud is warped between the move and the merge
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
                                                                             match_colors_gate=self.match_colors_gate, warp=self.warp)
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


# ---- geometric evaluation: depth maps of the two scenes from the same cameras, no photographs ---------------------
GEOMETRY_LOG_FIELDS = ("registration_data", "coverage", "depth_mae", "depth_rmse", "depth_rel", "depth_overlap", "per_camera", "error_list")
DEPTH_KEYS = ("depth_mae", "depth_rmse", "depth_rel", "depth_overlap")


def depth_agreement(d1, a1, d2, a2, coverage=0.5):
    """The depth agreement of two renders from one camera -> dict(depth_mae, depth_rmse, depth_rel, depth_overlap, n_mask, n_union), or
    ``None`` for the first three when the mask is empty.  ``mask = (a1 >= coverage) & (a2 >= coverage)``; over it the mean of
    ``|d1 - d2|``, the root mean square of ``d1 - d2`` and the mean of ``|d1 - d2| / ((d1 + d2) / 2)``; ``depth_overlap`` is the mask's
    size over that of ``(a1 >= coverage) | (a2 >= coverage)`` (``None`` when neither render covers a pixel).  Masked reductions in
    float64 with torch, wherever the maps live."""
    d1, a1, d2, a2 = (torch.as_tensor(x) for x in (d1, a1, d2, a2))
    c1, c2 = a1 >= coverage, a2 >= coverage
    mask, union = c1 & c2, c1 | c2
    n_mask, n_union = int(mask.sum()), int(union.sum())
    out = {"depth_mae": None, "depth_rmse": None, "depth_rel": None, "depth_overlap": n_mask / n_union if n_union else None, "n_mask": n_mask,
           "n_union": n_union}
    if n_mask:
        x, y = d1[mask].to(torch.float64), d2[mask].to(torch.float64)
        diff = x - y
        out["depth_mae"] = float(diff.abs().mean())
        out["depth_rmse"] = float(torch.sqrt((diff * diff).mean()))
        out["depth_rel"] = float((diff.abs() / (0.5 * (x + y))).mean())
    return out


@dataclass
class GeometryEvaluationObject:
    """One geometric evaluation: the means over the cameras with a non-empty mask, and every camera's own figures."""
    registration_data: dict = field(default_factory=dict)
    coverage: float = 0.5
    depth_mae: float = None
    depth_rmse: float = None
    depth_rel: float = None
    depth_overlap: float = None
    per_camera: list = field(default_factory=list)
    error_list: list = field(default_factory=list)

    def to_json(self):
        return {k: _json_value(getattr(self, k)) for k in GEOMETRY_LOG_FIELDS}


class GeometryEvaluator:
    """Does the surface of ``pc1`` moved by ``transformation`` coincide with that of ``pc2``?  Both are rendered SEPARATELY from every
    camera of ``cameras_list`` (``rasterize_depth``: expected depth and coverage) and compared where both cover the pixel
    (``depth_agreement``).  Needs no photographs; ``run()`` writes the JSON log ``GEOMETRY_LOG_FIELDS`` and polls ``cancel_evaluation``
    between cameras like ``RegistrationEvaluator``.  The two models are left as they were."""
    EvaluationObject = GeometryEvaluationObject

    def __init__(self, pc1, pc2, transformation, cameras_list, log_path, with_scaling=False, rotate_sh=False, coverage=0.5, registration_result=None,
                 warp=None):
        self.signal_cancel = False
        self.warp = warp                    # warp.WarpField or None: the first cloud is warped behind the move
        self.pc1, self.pc2 = pc1, pc2
        self.transformation = transformation
        self.cameras_list = cameras_list
        self.log_path = log_path
        self.with_scaling = bool(with_scaling)
        self.rotate_sh = rotate_sh
        self.coverage = float(coverage)
        self.registration_result = registration_result
        self.device = "cuda:0"
        self.per_camera = []
        self.current_progress = 0
        self.max_progress = len(cameras_list)

    def cancel_evaluation(self):
        self.signal_cancel = True

    def run(self):
        """-> the ``GeometryEvaluationObject`` written to ``log_path``, or ``None`` when cancelled (polled between cameras)."""
        moved = second = None               # moved and brought to the device at the first camera
        error_list, rows = [], []
        for camera in self.cameras_list:
            if self.signal_cancel:
                return None
            self.current_progress += 1
            if moved is None:
                moved = self.pc1.clone_gaussian()
                moved.move_to_device(self.device)
                if self.with_scaling:
                    moved.similarity_transform_gaussian_model(self.transformation, rotate_sh=self.rotate_sh)
                else:
                    moved.transform_gaussian_model(self.transformation, rotate_sh=self.rotate_sh)
                if self.warp is not None:
                    moved.warp_gaussian_model(self.warp)
                second = self.pc2
                if second.device_name != self.device:
                    second = second.clone_gaussian()
                    second.move_to_device(self.device)
            d1, a1 = rasterize_depth(moved, camera, 1, self.device)
            d2, a2 = rasterize_depth(second, camera, 1, self.device)
            row = dict(depth_agreement(d1, a1, d2, a2, self.coverage), image_name=camera.image_name)
            if row["n_mask"] == 0:
                error_list.append(f"{camera.image_name}: no pixel is covered (alpha >= {self.coverage:g}) by both scenes")
            rows.append(row)
        self.per_camera = rows
        used = [r for r in rows if r["n_mask"] > 0]
        mean = lambda k: float(np.mean([r[k] for r in used])) if used else None          # no camera compared: null in the log
        record = vars(self.registration_result) if self.registration_result is not None else {}
        evaluation = GeometryEvaluationObject(dict(record), self.coverage, *(mean(k) for k in DEPTH_KEYS), rows, error_list)
        with open(self.log_path, "w") as out:
            json.dump(evaluation.to_json(), out, indent=2, allow_nan=False)
        return evaluation
