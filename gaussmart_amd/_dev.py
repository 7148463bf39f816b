"""What every ctypes call into libgsr_hip.so needs from torch: pointers, the current stream, a workspace, and point clouds
brought to the device (or, for the host twins, to float64)."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def ptr(t):
    """Device (or host) address of a tensor; NULL for None and for an empty tensor."""
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(nbytes, dev):
    """Uninitialised bytes for a *_workspace_bytes() answer: at least one, so that the pointer is never NULL."""
    return torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=dev)


def device_points(points, device, who, keep_f64=False):
    """-> contiguous device tensor f32 [n,3].  keep_f64: float64 input stays float64 (anything else becomes f32) and the
    answer is (tensor, point_f64 flag)."""
    if isinstance(points, np.ndarray):
        if device is None:
            raise ValueError(f"{who}: a host array needs device=")
        host = np.float64 if keep_f64 and points.dtype == np.float64 else np.float32
        points = torch.from_numpy(np.ascontiguousarray(points, host)).to(device)
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _lib.GsrError(f"{who}: points must live on the device (no CPU path; see {who}_host)")
    if not (keep_f64 and points.dtype == torch.float64):
        points = points.to(torch.float32)
    points = points.contiguous()
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [n,3], got {list(points.shape)}")
    return (points, int(points.dtype == torch.float64)) if keep_f64 else points


def points64(points, keep_f64=False):
    """Host float64 [n,3] copy for the numpy twins, rounded through float32 like the device path (keep_f64: unless it is
    float64 already)."""
    p = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    if not (keep_f64 and p.dtype == np.float64):
        p = p.astype(np.float32)
    return np.ascontiguousarray(p.astype(np.float64).reshape(-1, 3))
