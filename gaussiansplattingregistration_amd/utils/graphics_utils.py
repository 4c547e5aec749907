"""``sh2rgb`` as in the reference's ``src/utils/graphics_utils.py:72-73`` (C0 = 0.28209479177387814) and ``getWorld2View2`` with the
meaning of ``:24-35`` (the 3DGS world -> camera matrix)."""
import numpy as np

C0 = 0.28209479177387814


def sh2rgb(sh):
    return sh * C0 + 0.5


def getWorld2View2(R, t, translate=np.array([0.0, 0.0, 0.0]), scale=1.0):
    """4x4 float32 world -> camera matrix ``[R^T | t]``, after the camera centre was moved by ``translate`` and scaled by ``scale``
    (both act on the camera-to-world side, hence the two inversions; they are kept for the defaults too so that the float32
    result is the reference's to the bit)."""
    view = np.zeros((4, 4))
    view[:3, :3] = np.asarray(R).transpose()
    view[:3, 3] = t
    view[3, 3] = 1.0
    pose = np.linalg.inv(view)
    pose[:3, 3] = (pose[:3, 3] + translate) * scale
    return np.linalg.inv(pose).astype(np.float32)
