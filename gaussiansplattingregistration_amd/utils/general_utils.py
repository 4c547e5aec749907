"""``convert_to_camera_transform`` with the meaning of the reference's ``src/utils/general_utils.py:83-91``."""
import numpy as np


def convert_to_camera_transform(rot, pos):
    """Camera-to-world pose (3x3 ``rot``, ``pos``) of a 3DGS ``cameras.json`` entry -> the ``(R, T)`` pair ``Camera`` takes: with
    ``[Rv | tv]`` the inverse of the pose (world -> camera), ``R = Rv^T`` and ``T = tv``."""
    pose = np.zeros((4, 4))
    pose[:3, :3] = rot
    pose[:3, 3] = pos
    pose[3, 3] = 1.0
    view = np.linalg.inv(pose)
    return view[:3, :3].transpose(), view[:3, 3]
