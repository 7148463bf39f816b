"""`simple_knn._C.distCUDA2` on top of libgsr_hip.so (call site scene/gaussian_model.py:22,261)."""
import torch

from . import _dev, _lib


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    """points f32 [N,3] on a HIP device -> f32 [N]: mean squared distance to the 3 nearest other
    points."""
    L = _lib.lib()
    if points.device.type != "cuda":
        raise _lib.GsrError("distCUDA2 needs a tensor on a HIP device (torch 'cuda'); there is no CPU path")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be [N,3]")
    pts = points.detach().float().contiguous()
    n = pts.shape[0]
    out = torch.empty((n,), dtype=torch.float32, device=pts.device)
    if n == 0:
        return out
    with torch.cuda.device(pts.device):
        ws = _dev.workspace(L.gsr_knn3_workspace_bytes(n), pts.device)
        _lib.check(L.gsr_knn3(_dev.ptr(pts), n, _dev.ptr(out), _dev.ptr(ws), ws.numel(), _dev.stream(pts.device)))
    return out


def sort_pairs_u32(keys: torch.Tensor, vals, begin_bit=0, end_bit=32):
    """Stable LSD radix sort of (key, value) pairs (int32 tensors viewed as u32); vals=None sorts
    indices.  Exposed for the bit-exactness tests of the binning sort."""
    L = _lib.lib()
    n = keys.numel()
    k = keys.contiguous()
    v = vals.contiguous() if vals is not None else None
    ko = torch.empty_like(k)
    vo = torch.empty_like(k)
    if n == 0:
        return ko, vo
    with torch.cuda.device(k.device):
        ws = _dev.workspace(L.gsr_sort_workspace_bytes(n), k.device)
        _lib.check(L.gsr_sort_pairs_u32(_dev.ptr(k), _dev.ptr(v) if v is not None else None, _dev.ptr(ko), _dev.ptr(vo), n,
                                        begin_bit, end_bit, _dev.ptr(ws), ws.numel(), _dev.stream(k.device)))
    return ko, vo
