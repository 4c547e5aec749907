"""Pinhole camera with the names of the reference's ``Camera`` (``src/models/camera.py:13-28``): ``viewmat (1,4,4)`` world -> camera,
``intrinsics (1,3,3)`` with the principal point at the image centre.  The viewer methods of the reference's class (rotate, zoom,
pan, roll) are GUI code and are not part of this backend.  ``load_cameras`` reads the ``cameras.json`` a 3DGS training run writes.
"""
from __future__ import annotations

import json

import numpy as np
import torch

from ..utils.general_utils import convert_to_camera_transform
from ..utils.graphics_utils import getWorld2View2


class Camera:
    def __init__(self, R, T, fx, fy, image_name, width, height):
        R, T = np.asarray(R, dtype=np.float64), np.asarray(T, dtype=np.float64)
        self.image_name, self.width, self.height = image_name, width, height
        self.rotation = torch.from_numpy(R.astype(np.float32))
        self.position = torch.from_numpy(T.astype(np.float32))
        K = np.eye(3, dtype=np.float32)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, width / 2, height / 2          # principal point: the image centre
        self.intrinsics = torch.from_numpy(K).unsqueeze(0)
        self.viewmat = torch.from_numpy(getWorld2View2(R, T)).unsqueeze(0)

    @property
    def fx(self):
        return float(self.intrinsics[0, 0, 0])

    @property
    def fy(self):
        return float(self.intrinsics[0, 1, 1])

    @property
    def cx(self):
        return float(self.intrinsics[0, 0, 2])

    @property
    def cy(self):
        return float(self.intrinsics[0, 1, 2])


def cameras_from_json(entries):
    """A list of ``Camera`` from the parsed entries of a ``cameras.json`` (fields ``fx fy width height rotation position img_name``:
    ``rotation`` / ``position`` are the camera-to-world pose), as the reference's Evaluation tab builds them
    (``src/gui/tabs/evaluation_tab.py:104-117``)."""
    cams = []
    for e in entries:
        rot = np.array([np.array(r) for r in e["rotation"]])
        pos = np.array([np.array(p) for p in e["position"]])
        R, T = convert_to_camera_transform(rot, pos)
        cams.append(Camera(R, T, e["fx"], e["fy"], e["img_name"], e["width"], e["height"]))
    return cams


def load_cameras(json_path):
    with open(json_path) as f:
        return cameras_from_json(json.load(f))
