"""Shared inputs and an independent restatement of LPIPS for tests/test_lpips_cpu.py and tests/test_gpu_lpips.py.

A golden vector from the reference is not possible: its lpipsPyTorch imports torchvision, which is not installed, and takes
its weights from the network.  So the torch twin (gaussmart_amd.lpips.lpips_host) is held to the restatement below, written
from the cited lines of the reference without F.conv2d / F.max_pool2d (unfold + matmul, strided slices), and the kernels
are held to the twin in fp64.

All weights are seeded random (gaussmart_amd.lpips.random_lpips_weights: convolutions randn * sqrt(2 / (C_in k^2)), biases
0.05 randn, linear weights rand / C); images are rand and rand plus clamped noise of sigma 0.1.  On these inputs every
tapped feature norm is above 1 (test_lpips_cpu checks it), so the + 1e-10 division is well conditioned.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from gaussmart_amd import lpips as LP


@functools.lru_cache(maxsize=None)
def weights(net_type):
    return LP.random_lpips_weights(net_type, seed=1234)


@functools.lru_cache(maxsize=None)
def image_pair(H, W, seed=0):
    """x = rand, y = clamp(x + 0.1 randn, 0, 1); float32 [3,H,W] on the CPU."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    x = torch.rand(3, H, W, generator=g)
    y = (x + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return x, y


@functools.lru_cache(maxsize=None)
def twin(net_type, H, W, dtype):
    """lpips_host of image_pair(H, W) in `dtype` on the CPU, as a Python float (computed once per session)."""
    x, y = image_pair(H, W)
    return float(LP.lpips_host(x.to(dtype), y.to(dtype), net_type=net_type, weights=weights(net_type)))


def tolerance(net_type, H, W):
    """The end-to-end rule: 4 * max(e_ref, 2^-23 |value|), e_ref = the fp32 CPU twin's own deviation from the fp64 twin."""
    v64, v32 = twin(net_type, H, W, torch.float64), twin(net_type, H, W, torch.float32)
    return 4.0 * max(abs(v32 - v64), 2.0 ** -23 * abs(v64))


# ---------------------------------------------------------------- the restatement
def _conv_restated(x, w, b, stride, pad):
    """nn.Conv2d as a matrix product over unfolded patches (zero padding)."""
    B, _, H, W = x.shape
    co, ci, k, _ = w.shape
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(x, kernel_size=k, padding=pad, stride=stride)            # [B, ci k k, oh ow]
    out = w.reshape(co, ci * k * k) @ cols + b[None, :, None]
    return out.reshape(B, co, oh, ow)


def _pool_restated(x, k):
    """nn.MaxPool2d(k, stride 2), floor mode, no padding: the maximum of the k*k strided slices."""
    H, W = x.shape[-2:]
    oh, ow = (H - k) // 2 + 1, (W - k) // 2 + 1
    out = None
    for dy in range(k):
        for dx in range(k):
            s = x[..., dy:dy + 2 * (oh - 1) + 1:2, dx:dx + 2 * (ow - 1) + 1:2]
            out = s if out is None else torch.maximum(out, s)
    return out


# torchvision's `features` as (kind, argument) lists, truncated where BaseNet.forward stops (modules/networks.py:53-63):
# 'c' = the next convolution (kernel, stride, pad), 'r' = relu, 'p' = max-pool window; target_layers count from 1
_ALEX_LAYERS = [("c", (11, 4, 2)), ("r", None), ("p", 3), ("c", (5, 1, 2)), ("r", None), ("p", 3), ("c", (3, 1, 1)), ("r", None),
                ("c", (3, 1, 1)), ("r", None), ("c", (3, 1, 1)), ("r", None)]
_ALEX_TARGETS = [2, 5, 8, 10, 12]
_VGG_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512]
_VGG_TARGETS = [4, 9, 16, 23, 30]


def restated_features(x, w):
    """BaseNet.forward: z-score, walk the layers, collect normalize_activation(x) at the target layers."""
    mean = torch.tensor([-.030, -.088, -.188])[None, :, None, None].to(x.dtype)
    std = torch.tensor([.458, .448, .450])[None, :, None, None].to(x.dtype)
    x = (x - mean) / std
    if w.net_type == "alex":
        layers, targets = _ALEX_LAYERS, _ALEX_TARGETS
    else:
        layers, targets = [], _VGG_TARGETS
        for v in _VGG_CFG:
            layers += [("p", 2)] if v == "M" else [("c", (3, 1, 1)), ("r", None)]
    out, n_conv = [], 0
    for i, (kind, arg) in enumerate(layers, 1):
        if kind == "c":
            x = _conv_restated(x, w.conv_w[n_conv].to(x.dtype), w.conv_b[n_conv].to(x.dtype), arg[1], arg[2])
            n_conv += 1
        elif kind == "r":
            x = x.clamp(min=0)
        else:
            x = _pool_restated(x, arg)
        if i in targets:
            norm = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
            out.append((x / (norm + 1e-10), norm))
    return out


def restated_lpips(x, y, w):
    """LPIPS.forward (modules/lpips.py:30-36) on [1,3,H,W] inputs; -> ([1,1,1,1] value, the smallest tapped feature norm)."""
    fx, fy = restated_features(x, w), restated_features(y, w)
    res, min_norm = [], float("inf")
    for k, ((a, na), (b, nb)) in enumerate(zip(fx, fy)):
        d = (a - b) ** 2
        res.append((d * w.lin[k].to(x.dtype)[None, :, None, None]).sum(1, keepdim=True).mean((2, 3), True))
        min_norm = min(min_norm, float(na.min()), float(nb.min()))
    return torch.sum(torch.cat(res, 0), 0, True), min_norm


# ---------------------------------------------------------------- files for the loader and metrics_cli
def write_weight_files(tmp_path, net_type, extra=True):
    """The two files in torchvision / LPIPS v0.1 naming, from the seeded weights."""
    w = weights(net_type)
    trunk = {}
    for i, cw, cb in zip(LP.FEATURE_INDEX[net_type], w.conv_w, w.conv_b):
        trunk[f"features.{i}.weight"], trunk[f"features.{i}.bias"] = cw, cb
    if extra:
        trunk["classifier.0.weight"], trunk["classifier.0.bias"] = torch.zeros(4, 4), torch.zeros(4)
    names = LP.DIR_FILES[net_type]
    backbone, lin = str(tmp_path / names[0][0]), str(tmp_path / names[1][0])
    torch.save(trunk, backbone)
    torch.save({f"lin{k}.model.1.weight": v.reshape(1, -1, 1, 1) for k, v in enumerate(w.lin)}, lin)
    return backbone, lin


def write_model(root, n=3, H=40, W=56, method="ours_30000"):
    """A MODEL directory as render_cli leaves it: test/<method>/{renders,gt}/NNNNN.png, written in unsorted order."""
    from PIL import Image
    g = torch.Generator().manual_seed(5)
    for sub in ("renders", "gt"):
        os.makedirs(os.path.join(root, "test", method, sub), exist_ok=True)
    names = []
    for i in (2, 0, 1)[:n]:
        gt = torch.rand(H, W, 4 if i == 0 else 3, generator=g)          # one ground truth carries an alpha channel
        rd = (gt[..., :3] + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
        name = f"{i:05d}.png"
        Image.fromarray((gt.numpy() * 255).astype(np.uint8)).save(os.path.join(root, "test", method, "gt", name))
        Image.fromarray((rd.numpy() * 255).astype(np.uint8)).save(os.path.join(root, "test", method, "renders", name))
        names.append(name)
    return sorted(names)


def load_pair(root, method, name):
    from PIL import Image
    out = []
    for sub in ("renders", "gt"):
        a = np.asarray(Image.open(os.path.join(root, "test", method, sub, name)))
        out.append((torch.from_numpy(a.copy()).permute(2, 0, 1)[:3].float() / 255.0)[None])
    return out
