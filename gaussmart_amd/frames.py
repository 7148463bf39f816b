"""Pictures from the maps of a render package, next to the maps (gsr_frame_*, include/gsr.h FRAME_*): the 8-bit frames the
exports and videos write (utils/render_utils.py: save_img_u8, create_videos) and the viewer pictures of utils/image_utils.py
(gradient_map, colormap, render_net_image).  Every device function has a `*_host` twin: numpy with explicit dtypes for the
u8 and turbo paths, torch on the CPU for gradient_map and colormap.

    from gaussmart_amd.frames import to_u8, depth_limits, depth_to_turbo, render_net_image, RENDER_ITEMS
    rgb = to_u8(pkg["render"])                                  # u8 [H,W,3] on the device
    lo, hi = depth_limits(pkg["surf_depth"])                    # log of the 3 % / 97 % depth
    clean, frame = depth_to_turbo(pkg["surf_depth"], lo, hi)    # fp32 depth for the TIFF, u8 [H,W,3] video frame
    edge = render_net_image(pkg, RENDER_ITEMS, 4, camera)       # f32 [3,H,W]
"""
import ctypes as C

import numpy as np
import torch

from . import _dev, _lib
from .colormaps import turbo_f32, turbo_u8

RENDER_ITEMS = ['RGB', 'Alpha', 'Normal', 'Depth', 'Edge', 'Curvature']

_tables = {}


def _table(kind, dev):
    """The turbo table on `dev`: "u8" [256,3] bytes of a video frame, "f32" [256,3] colours of colormap()."""
    key = (kind, str(dev))
    if key not in _tables:
        _tables[key] = torch.from_numpy(turbo_u8() if kind == "u8" else turbo_f32()).to(dev).contiguous()
    return _tables[key]


def _device_f32(x, who):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.GsrError(f"{who}: the map must live on the device (no CPU path; see {who}_host)")
    return x.detach().to(torch.float32).contiguous()


# ---------------------------------------------------------------- u8 frames
def to_u8(x):
    """uint8(clip(nan_to_num(x), 0, 1) * 255) of a device map f32 [B,C,H,W] or [C,H,W], C in {1, 3, 4}, as u8 [B,H,W,C] or
    [H,W,C]: the bytes mesh._save_img_u8 writes (gsr_frame_to_u8)."""
    x = _device_f32(x, "to_u8")
    if x.dim() not in (3, 4):
        raise ValueError(f"to_u8: the map must be [C,H,W] or [B,C,H,W], got {list(x.shape)}")
    B, (Cn, H, W) = (x.shape[0] if x.dim() == 4 else 1), x.shape[-3:]
    out = torch.empty((B, H, W, Cn), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().gsr_frame_to_u8(_dev.ptr(x), B, Cn, H, W, _dev.ptr(out), _dev.stream(x.device)))
    return out if x.dim() == 4 else out[0]


def to_u8_host(x):
    """numpy twin of to_u8: float32 in, one float32 multiply, truncation."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float32)
    x = np.moveaxis(x, -3, -1)
    return (np.clip(np.nan_to_num(x), np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)


# ---------------------------------------------------------------- depth limits and the turbo depth frame
def _percentile_ranks(n, qs):
    """numpy's method="linear" (numpy/lib/_function_base_impl.py: _compute_virtual_index, _get_indexes, _get_gamma) for
    percentiles qs of n values: per percentile the two neighbouring ranks and the weight of the upper one, in float64 and in
    numpy's own order of operations (n q + (1 - q) - 1, not (n - 1) q)."""
    out = []
    for q in np.true_divide(np.asarray(qs, np.float64), 100):
        v = n * q + (1 + q * (1 - 1 - 1)) - 1
        if v >= n - 1:
            lo = hi = n - 1
        elif v < 0:
            lo = hi = 0
        else:
            lo = int(np.floor(v))
            hi = lo + 1
        out.append((lo, hi, v - np.floor(v)))
    return out


def _lerp_log(stats, ranks):
    """log of numpy's _lerp over the float32 order statistics [a0, b0, a1, b1]: the difference b - a in the values' own
    float32, the products and sums in float64, from the upper end where the weight is >= 0.5."""
    a, b = np.asarray(stats[0::2], np.float32), np.asarray(stats[1::2], np.float32)
    g = np.asarray([r[2] for r in ranks], np.float64)
    with np.errstate(all="ignore"):
        d = np.subtract(b, a)
        lims = np.where(g >= 0.5, b - d * (1 - g), a + d * g)
        lo, hi = (float(x) for x in np.log(lims))
    return lo, hi


def order_stats(values, ranks):
    """The elements at `ranks` (0-based, at most 8) of the ascending nan_to_num(values), as float32 numpy: a device sort and
    ONE read-back of len(ranks) floats (gsr_frame_order_stats)."""
    v = _device_f32(values, "order_stats").reshape(-1)
    n, k = v.numel(), len(ranks)
    L = _lib.lib()
    ws = _dev.workspace(L.gsr_frame_order_stats_workspace_bytes(n), v.device)
    r = (C.c_int64 * k)(*[int(x) for x in ranks])
    out = (C.c_float * k)()
    with torch.cuda.device(v.device):
        _lib.check(L.gsr_frame_order_stats(_dev.ptr(v), n, r, k, out, _dev.ptr(ws), ws.numel(), _dev.stream(v.device)))
    return np.array(list(out), np.float32)


def depth_limits(depth, p=3):
    """(lo, hi) = log of the p-th and (100 - p)-th percentile of nan_to_num(depth) (create_videos: distance_limits): the four
    order statistics come from the device, numpy's linear interpolation runs here in float64."""
    n = depth.numel()
    ranks = _percentile_ranks(n, (p, 100 - p))
    stats = order_stats(depth, [r for lo, hi, _ in ranks for r in (lo, hi)])
    return _lerp_log(stats, ranks)


def depth_limits_host(depth, p=3):
    d = np.nan_to_num(np.asarray(depth.detach().cpu().numpy() if isinstance(depth, torch.Tensor) else depth, np.float32))
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, hi = (float(np.log(x)) for x in np.percentile(d.flatten(), [p, 100 - p]))
    return lo, hi


def depth_to_turbo(depth, lo, hi, want_clean=True):
    """(clean, frame) of a device depth map f32 [B,1,H,W], [1,H,W] or [H,W]: clean = nan_to_num(depth) as fp32 in the same
    shape (None with want_clean=False), frame = the turbo video frame u8 [B,H,W,3] ([H,W,3] without a batch) of
    clip((log(clean) - min(lo, hi)) / |hi - lo|, 0, 1) (gsr_frame_depth_vis)."""
    d = _device_f32(depth, "depth_to_turbo")
    if d.dim() == 4:
        B, H, W = d.shape[0], d.shape[2], d.shape[3]
    else:
        B, (H, W) = 1, d.shape[-2:]
    if d.numel() != B * H * W:
        raise ValueError(f"depth_to_turbo: the depth must have one channel, got {list(d.shape)}")
    clean = torch.empty_like(d) if want_clean else None
    frame = torch.empty((B, H, W, 3), dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        _lib.check(_lib.lib().gsr_frame_depth_vis(_dev.ptr(d), B, H, W, float(lo), float(hi), _dev.ptr(_table("u8", d.device)),
                                                  _dev.ptr(clean), _dev.ptr(frame), _dev.stream(d.device)))
    return clean, (frame if d.dim() == 4 else frame[0])


def clean_depth(depth):
    """nan_to_num(depth) as fp32 on the device, the payload of a depth TIFF (gsr_frame_depth_vis without a frame)."""
    d = _device_f32(depth, "clean_depth")
    clean = torch.empty_like(d)
    with torch.cuda.device(d.device):
        _lib.check(_lib.lib().gsr_frame_depth_vis(_dev.ptr(d), 1, 1, d.numel(), 0.0, 1.0, _dev.ptr(_table("u8", d.device)),
                                                  _dev.ptr(clean), None, _dev.stream(d.device)))
    return clean


def depth_turbo_index_host(depth, lo, hi, log_dtype=np.float32):
    """(clean float32, index int64) of a depth array: the row of the turbo table every pixel of the video frame takes, -1
    where the normalised value is NaN (create_videos:262-263 and the lookup of matplotlib's Colormap.__call__ written
    out: trunc(t * 256), 256 -> 255).  The log is taken in log_dtype (the reference: the frame's float32); the
    normalisation runs in float64, as numpy 2 promotes it through the float64 limits."""
    d = np.nan_to_num(np.asarray(depth.detach().cpu().numpy() if isinstance(depth, torch.Tensor) else depth, np.float32))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log(d.astype(log_dtype)).astype(np.float64)
        t = np.clip((t - np.minimum(np.float64(lo), np.float64(hi))) / np.abs(np.float64(hi) - np.float64(lo)), 0, 1)
    bad = np.isnan(t)
    idx = np.minimum((np.where(bad, 0.0, t) * 256.0).astype(np.int64), 255)
    return d, np.where(bad, -1, idx)


def depth_to_turbo_host(depth, lo, hi):
    """numpy twin of depth_to_turbo: (clean float32, frame u8 [...,3]); a NaN pixel is black."""
    d, idx = depth_turbo_index_host(depth, lo, hi)
    frame = turbo_u8()[np.maximum(idx, 0)]
    frame[idx < 0] = 0
    return d, frame


# ---------------------------------------------------------------- gradient_map, colormap, render_net_image
def gradient_map(image):
    """utils/image_utils.py:23-32 on a device image f32 [C,H,W] -> [1,H,W]: Sobel magnitude per channel (zero padding,
    kernels / 4), L2 norm over the channels (gsr_frame_sobel: one launch, a fixed order of sums)."""
    x = _device_f32(image, "gradient_map")
    if x.dim() != 3:
        raise ValueError(f"gradient_map: the image must be [C,H,W], got {list(x.shape)}")
    Cn, H, W = x.shape
    out = torch.empty((1, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().gsr_frame_sobel(_dev.ptr(x), Cn, H, W, _dev.ptr(out), _dev.stream(x.device)))
    return out


def gradient_map_host(image):
    """The reference's formulation with torch on the CPU (F.conv2d)."""
    import torch.nn.functional as F
    image = image.detach().cpu().float()
    sobel_x = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]).float().unsqueeze(0).unsqueeze(0) / 4
    sobel_y = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]]).float().unsqueeze(0).unsqueeze(0) / 4
    grad_x = torch.cat([F.conv2d(image[i].unsqueeze(0), sobel_x, padding=1) for i in range(image.shape[0])])
    grad_y = torch.cat([F.conv2d(image[i].unsqueeze(0), sobel_y, padding=1) for i in range(image.shape[0])])
    magnitude = torch.sqrt(grad_x ** 2 + grad_y ** 2)
    return magnitude.norm(dim=0, keepdim=True)


def colormap(map, cmap="turbo"):
    """utils/image_utils.py:34-39 on a device map f32 [1,H,W] (or [H,W]) -> f32 [3,H,W]: min and max by gsr_frame_minmax
    (no read-back), then gsr_frame_colormap.  DEVIATION: a constant map gives the table's first colour everywhere (the
    reference divides 0 by 0 and converts NaN to an integer)."""
    if cmap != "turbo":
        raise ValueError(f"colormap: only 'turbo' is tabulated (gaussmart_amd/colormaps.py), got {cmap!r}")
    x = _device_f32(map, "colormap")
    H, W = x.shape[-2:]
    if x.numel() != H * W or x.numel() == 0:
        raise ValueError(f"colormap: the map must be a non-empty [1,H,W] or [H,W], got {list(x.shape)}")
    L = _lib.lib()
    bounds = torch.empty(2, dtype=torch.int32, device=x.device)
    out = torch.empty((3, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        s = _dev.stream(x.device)
        _lib.check(L.gsr_frame_minmax(_dev.ptr(x), H * W, _dev.ptr(bounds), s))
        _lib.check(L.gsr_frame_colormap(_dev.ptr(x), H, W, _dev.ptr(bounds), _dev.ptr(_table("f32", x.device)), _dev.ptr(out), s))
    return out


def colormap_host(map, cmap="turbo"):
    """torch twin on the CPU (float32, the reference's operations), with colormap's rule for a constant map."""
    if cmap != "turbo":
        raise ValueError(f"colormap_host: only 'turbo' is tabulated, got {cmap!r}")
    map = map.detach().cpu().float()
    colors = torch.from_numpy(turbo_f32())
    H, W = map.shape[-2:]
    lo, hi = map.min(), map.max()
    if bool(hi == lo):
        idx = torch.zeros((H, W), dtype=torch.long)
    else:
        idx = ((map - lo) / (hi - lo) * 255).round().long().reshape(H, W)
    return colors[idx].permute(2, 0, 1).contiguous()


def _net_image(render_pkg, render_items, render_mode, grad, cmap):
    output = render_items[render_mode].lower()
    if output == 'alpha':
        net_image = render_pkg["rend_alpha"]
    elif output == 'normal':
        net_image = (render_pkg["rend_normal"] + 1) / 2
    elif output == 'depth':
        net_image = render_pkg["surf_depth"]
    elif output == 'edge':
        net_image = grad(render_pkg["render"])
    elif output == 'curvature':
        net_image = grad((render_pkg["rend_normal"] + 1) / 2)
    else:
        net_image = render_pkg["render"]
    if net_image.shape[0] == 1:
        net_image = cmap(net_image)
    return net_image


def render_net_image(render_pkg, render_items, render_mode, camera):
    """utils/image_utils.py:41-61: the picture of render_items[render_mode] (RENDER_ITEMS) as f32 [3,H,W]; one-channel maps
    (alpha, depth, edge, curvature) go through colormap.  `camera` is not read, as in the reference."""
    return _net_image(render_pkg, render_items, render_mode, gradient_map, colormap)


def render_net_image_host(render_pkg, render_items, render_mode, camera):
    return _net_image({k: v.detach().cpu() for k, v in render_pkg.items() if isinstance(v, torch.Tensor)}, render_items,
                      render_mode, gradient_map_host, colormap_host)
