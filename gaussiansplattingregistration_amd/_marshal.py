"""What crosses the C ABI from Python: numpy arrays (staged through host memory by the library) or PyTorch-ROCm tensors on the
device (zero-copy: only ``data_ptr()`` crosses).  One place for the ctypes fronts (``hem``, ``icp``, ``voxel``, ``features``, ...).
"""
from __future__ import annotations

import numpy as np

try:  # torch is optional for host-array use
    import torch
except Exception:  # pragma: no cover
    torch = None


def is_tensor(a):
    return torch is not None and isinstance(a, torch.Tensor)


def is_cuda(a):
    return is_tensor(a) and a.is_cuda


def _torch_dtype(dtype):
    return getattr(torch, np.dtype(dtype).name)


def prep(a, shape, dtype, device):
    """-> (pointer, keep-alive, on_device) of a contiguous array of ``shape`` and ``dtype``: a tensor on cuda:``device`` in place,
    anything else (host tensor, ndarray, list) as a numpy array.  ``None`` -> (None, None, None)."""
    if a is None:
        return None, None, None
    if is_cuda(a):
        if a.device.index != device:
            raise RuntimeError(f"tensor lives on {a.device}, requested cuda:{device}")
        t = a.detach().to(_torch_dtype(dtype)).reshape(shape).contiguous()
        return t.data_ptr(), t, True
    if is_tensor(a):
        a = a.detach().cpu().numpy()
    arr = np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(shape))
    return arr.ctypes.data, arr, False


def out(shape, dtype, device, on_device):
    """-> (uninitialised tensor on cuda:``device`` or numpy array, pointer) for the library to write"""
    if on_device:
        t = torch.empty(shape, dtype=_torch_dtype(dtype), device=torch.device("cuda", device))
        return t, t.data_ptr()
    a = np.empty(shape, dtype)
    return a, a.ctypes.data


def stream_ptr(device, on_device):
    """torch's current stream on the device for device arrays, the null stream for host arrays"""
    return torch.cuda.current_stream(device).cuda_stream if on_device else 0
