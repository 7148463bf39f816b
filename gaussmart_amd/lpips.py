"""LPIPS on the device: the reference's lpipsPyTorch (called at metrics.py:73 and train.py:70,326) with its names and argument
meaning, computed by the kernels of csrc/lpips.hip (include/gsr.h: LP_CONV, LP_POOL, LP_HEAD, LP_FORWARD).

    from gaussmart_amd.lpips import LPIPS, lpips, load_lpips_weights
    weights = load_lpips_weights("vgg", "vgg16.pth", "vgg.pth")          # two LOCAL files, see below
    d = lpips(render, gt, net_type="vgg", weights=weights)               # [1,1,1,1], as the reference returns it
    criterion = LPIPS(net_type="alex", version="0.1", weights=...)       # train.py's form; criterion(x, y)

What differs from the reference, on purpose:
  * nothing is fetched.  The reference takes the trunk from torchvision's model zoo and the five linear layers from a URL
    (modules/networks.py:81,92 and modules/utils.py:13-20); here both are files the user supplies: the torchvision-format
    state dict of the trunk (vgg16 / alexnet: keys features.<i>.weight|bias) and the LPIPS v0.1 file of the linear layers
    (keys lin<k>.model.1.weight).  torchvision itself is not needed.
  * inputs go in as given, [3,H,W] or [1,3,H,W]; a batch above 1 is refused (the reference's cat(..., 0).sum(0) would silently
    ADD the batch), 'squeeze' is refused, CPU tensors are refused: `lpips_host` is the torch formulation of the same layers
    (any dtype, any device), which serves metrics_cli --host and the tests.
"""
import ctypes as C
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

from . import _lib
from ._dev import ptr, stream, workspace

# torchvision's `features` indices of the convolutions (models.vgg16 / models.alexnet)
FEATURE_INDEX = {"vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), "alex": (0, 3, 6, 8, 10)}
# per convolution: C_in, C_out, kernel, stride, pad, window of the max-pool in front of it (0: none), tapped after its relu?
TRUNK = {
    "alex": ((3, 64, 11, 4, 2, 0, True), (64, 192, 5, 1, 2, 3, True), (192, 384, 3, 1, 1, 3, True), (384, 256, 3, 1, 1, 0, True),
             (256, 256, 3, 1, 1, 0, True)),
    "vgg": ((3, 64, 3, 1, 1, 0, False), (64, 64, 3, 1, 1, 0, True),
            (64, 128, 3, 1, 1, 2, False), (128, 128, 3, 1, 1, 0, True),
            (128, 256, 3, 1, 1, 2, False), (256, 256, 3, 1, 1, 0, False), (256, 256, 3, 1, 1, 0, True),
            (256, 512, 3, 1, 1, 2, False), (512, 512, 3, 1, 1, 0, False), (512, 512, 3, 1, 1, 0, True),
            (512, 512, 3, 1, 1, 2, False), (512, 512, 3, 1, 1, 0, False), (512, 512, 3, 1, 1, 0, True)),
}
N_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}      # modules/networks.py:84,95
MIN_SIZE = {"alex": 31, "vgg": 16}
_NET_ID = {"alex": _lib.GSR_LPIPS_ALEX, "vgg": _lib.GSR_LPIPS_VGG}
# BaseNet.__init__ (modules/networks.py:41-44): float32 buffers
Z_MEAN = (-.030, -.088, -.188)
Z_STD = (.458, .448, .450)
# file names looked for in a weights directory: the trunk (torchvision's own download names too), then the linear layers
DIR_FILES = {"vgg": (("vgg16.pth", "vgg16-397923af.pth"), ("vgg.pth",)),
             "alex": (("alexnet.pth", "alexnet-owt-7be5be79.pth"), ("alex.pth",))}


def _check_net(net_type):
    if net_type == "squeeze":
        raise NotImplementedError("lpips: net_type 'squeeze' is not built; choose 'alex' or 'vgg'")
    if net_type not in TRUNK:
        raise NotImplementedError("choose net_type from [alex, vgg].")


class LpipsWeights:
    """The trunk's convolutions (conv_w[l] [C_out,C_in,k,k], conv_b[l] [C_out]) and the five linear layers (lin[k] [C_k])."""

    def __init__(self, net_type, conv_w, conv_b, lin):
        _check_net(net_type)
        spec = TRUNK[net_type]
        if len(conv_w) != len(spec) or len(conv_b) != len(spec) or len(lin) != 5:
            raise ValueError(f"lpips weights: {net_type} has {len(spec)} convolutions and 5 linear layers")
        for l, (ci, co, k, _, _, _, _) in enumerate(spec):
            if tuple(conv_w[l].shape) != (co, ci, k, k) or tuple(conv_b[l].shape) != (co,):
                raise ValueError(f"lpips weights: convolution {l} of {net_type} must be [{co},{ci},{k},{k}] with bias [{co}], got "
                                 f"{list(conv_w[l].shape)} and {list(conv_b[l].shape)}")
        lin = [w.reshape(-1) for w in lin]
        for k, c in enumerate(N_CHANNELS[net_type]):
            if lin[k].numel() != c:
                raise ValueError(f"lpips weights: linear layer {k} of {net_type} must have {c} weights, got {lin[k].numel()}")
        self.net_type, self.conv_w, self.conv_b, self.lin = net_type, list(conv_w), list(conv_b), lin
        self._criterion = None      # lpips() keeps its LPIPS of these weights here

    def to(self, device=None, dtype=None):
        f = lambda t: t.detach().to(device=device, dtype=dtype).contiguous()
        return LpipsWeights(self.net_type, [f(t) for t in self.conv_w], [f(t) for t in self.conv_b], [f(t) for t in self.lin])


def load_lpips_weights(net_type, backbone_path, lin_path):
    """Reads the two local files (torch.load(..., weights_only=True)); nothing here opens a URL."""
    _check_net(net_type)
    missing = [p for p in (backbone_path, lin_path) if not (p and os.path.isfile(p))]
    if missing:
        raise FileNotFoundError(
            f"lpips: {', '.join(map(str, missing))} not found.  LPIPS needs two local files (nothing is downloaded): the "
            f"torchvision-format state dict of the {'vgg16' if net_type == 'vgg' else 'alexnet'} trunk (got {backbone_path}) and "
            f"the LPIPS v0.1 linear layers {net_type}.pth (got {lin_path})")
    trunk = torch.load(backbone_path, map_location="cpu", weights_only=True)
    conv_w, conv_b = [], []
    for i in FEATURE_INDEX[net_type]:               # classifier.* and anything else is ignored
        for name, dst in ((f"features.{i}.weight", conv_w), (f"features.{i}.bias", conv_b)):
            if name not in trunk:
                raise KeyError(f"{backbone_path}: no key {name} (a torchvision {net_type} state dict is expected)")
            dst.append(trunk[name].float())
    lin_sd = OrderedDict()
    for key, val in torch.load(lin_path, map_location="cpu", weights_only=True).items():
        lin_sd[key.replace("lin", "").replace("model.", "")] = val          # get_state_dict (modules/utils.py:22-28)
    lin = []
    for k in range(5):
        if f"{k}.1.weight" not in lin_sd:
            raise KeyError(f"{lin_path}: no key lin{k}.model.1.weight (the LPIPS v0.1 file of {net_type} is expected)")
        lin.append(lin_sd[f"{k}.1.weight"].float())
    return LpipsWeights(net_type, conv_w, conv_b, lin)


def weights_from_dir(net_type, directory):
    """load_lpips_weights on the files of one directory: see DIR_FILES for the names."""
    _check_net(net_type)
    paths = []
    for names in DIR_FILES[net_type]:
        found = [os.path.join(directory, n) for n in names if os.path.isfile(os.path.join(directory, n))]
        paths.append(found[0] if found else os.path.join(directory, names[0]))
    return load_lpips_weights(net_type, *paths)


def random_lpips_weights(net_type, seed=0):
    """Seeded stand-ins of the right shapes and scale (He-initialised convolutions, small biases, positive linear weights):
    what the benchmark and the tests run on, since no trained file may be assumed."""
    _check_net(net_type)
    g = torch.Generator().manual_seed(seed)
    conv_w, conv_b = [], []
    for ci, co, k, _, _, _, _ in TRUNK[net_type]:
        conv_w.append(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
        conv_b.append(0.05 * torch.randn(co, generator=g))
    lin = [torch.rand(c, generator=g) / c for c in N_CHANNELS[net_type]]
    return LpipsWeights(net_type, conv_w, conv_b, lin)


def _resolve(net_type, weights):
    if isinstance(weights, LpipsWeights):
        if weights.net_type != net_type:
            raise ValueError(f"lpips: weights of {weights.net_type!r} given for net_type {net_type!r}")
        return weights
    if isinstance(weights, (str, os.PathLike)):
        return weights_from_dir(net_type, os.fspath(weights))
    if isinstance(weights, (tuple, list)) and len(weights) == 2:
        return load_lpips_weights(net_type, *weights)
    raise FileNotFoundError(
        "lpips: weights= is required (nothing is downloaded): an LpipsWeights, a directory holding "
        f"{DIR_FILES[net_type][0][0]} and {DIR_FILES[net_type][1][0]}, or the pair (backbone_path, lin_path)")


def _pair(x, y, who):
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError(f"{who}: x and y must be tensors")
    out = []
    for t in (x, y):
        if t.dim() == 4:
            if t.shape[0] != 1:
                raise ValueError(f"{who}: a batch of {t.shape[0]} is refused (the reference would add the batch's distances); "
                                 "call once per pair")
            t = t[0]
        if t.dim() != 3:
            raise ValueError(f"{who}: expected [3,H,W] or [1,3,H,W], got {list(t.shape)}")
        out.append(t)
    if out[0].shape != out[1].shape:
        raise ValueError(f"{who}: shapes differ: {list(out[0].shape)} vs {list(out[1].shape)}")
    return out


class LPIPS(torch.nn.Module):
    """criterion(x, y) -> [1,1,1,1]; the reference's class (modules/lpips.py:8-36) on the kernels."""

    def __init__(self, net_type="alex", version="0.1", weights=None):
        assert version in ["0.1"], "v0.1 is only supported now"
        super().__init__()
        _check_net(net_type)
        self.net_type = net_type
        self.weights = _resolve(net_type, weights)
        self._on = {}           # device -> (LpipsWeights there, the three host tables of device pointers)

    def _device_weights(self, dev):
        hit = self._on.get(dev)
        if hit is None:
            w = self.weights.to(dev, torch.float32)
            tables = [(C.c_void_p * len(ts))(*[t.data_ptr() for t in ts]) for ts in (w.conv_w, w.conv_b, w.lin)]
            hit = self._on[dev] = (w, tables)
        return hit

    @torch.no_grad()
    def forward(self, x, y):
        x, y = _pair(x, y, "lpips")
        if not x.is_cuda or not y.is_cuda:
            raise _lib.GsrError("lpips: tensors must live on the device (no CPU path; see lpips_host)")
        x = x.detach().to(torch.float32).contiguous()
        y = y.detach().to(device=x.device, dtype=torch.float32).contiguous()
        ch, H, W = (int(v) for v in x.shape)
        L = _lib.lib()
        _, (tw, tb, tl) = self._device_weights(x.device)
        net = _NET_ID[self.net_type]
        nbytes = L.gsr_lpips_workspace_bytes(net, H, W)
        ws = workspace(nbytes, x.device)
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        _lib.check(L.gsr_lpips_forward(net, tw, tb, tl, ptr(x), ptr(y), ch, H, W, ptr(ws), nbytes, ptr(out), stream(x.device)))
        return out.reshape(1, 1, 1, 1)


def lpips(x, y, net_type="alex", version="0.1", weights=None):
    """The reference's function (lpipsPyTorch/__init__.py:6-21).  For an LpipsWeights object the criterion is built once and
    kept ON that object, so it (and its device copies) goes when the caller drops the weights; there is no module-level
    cache.  For paths the criterion is built on every call, as the reference does, so files that change are read again --
    hold an LPIPS, or load the weights once, in a loop."""
    if not isinstance(weights, LpipsWeights):
        return LPIPS(net_type, version, weights)(x, y)
    crit = weights._criterion
    if crit is None or crit.net_type != net_type:           # the other net with these weights: the constructor refuses it
        crit = weights._criterion = LPIPS(net_type, version, weights)
    return crit(x, y)


def trunk_features_host(x, weights):
    """The tapped activations (after their relus) of x [B,3,H,W], in x's dtype on x's device: BaseNet.forward without the
    normalisation (modules/networks.py:53-63)."""
    w = weights.to(x.device, x.dtype)
    mean = torch.tensor(Z_MEAN, dtype=torch.float32, device=x.device).to(x.dtype)[None, :, None, None]
    std = torch.tensor(Z_STD, dtype=torch.float32, device=x.device).to(x.dtype)[None, :, None, None]
    x = (x - mean) / std
    taps = []
    for l, (_, _, _, stride, pad, pool, tap) in enumerate(TRUNK[weights.net_type]):
        if pool:
            x = F.max_pool2d(x, kernel_size=pool, stride=2)
        x = F.relu(F.conv2d(x, w.conv_w[l], w.conv_b[l], stride=stride, padding=pad))
        if tap:
            taps.append(x)
    return taps


def head_host(fx, fy, lin_w):
    """One layer's value [1,1,1,1] from the two maps [1,C,H,W]: normalize_activation (modules/utils.py:6-8), the squared
    difference, the 1x1 convolution and the spatial mean (modules/lpips.py:33-34)."""
    nx = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10)
    return F.conv2d((nx - ny) ** 2, lin_w.to(fx.dtype).reshape(1, -1, 1, 1)).mean((2, 3), True)


@torch.no_grad()
def lpips_host(x, y, net_type="alex", version="0.1", weights=None):
    """The torch twin: same layers through F.conv2d / F.max_pool2d, in the dtype and on the device of x."""
    assert version in ["0.1"], "v0.1 is only supported now"
    _check_net(net_type)
    weights = _resolve(net_type, weights)
    x, y = _pair(x, y, "lpips_host")
    if x.shape[0] != 3:
        raise ValueError(f"lpips_host: images must have 3 channels (got {x.shape[0]})")
    if min(x.shape[1:]) < MIN_SIZE[net_type]:
        raise ValueError(f"lpips_host: a {x.shape[1]}x{x.shape[2]} image is below the {net_type} trunk's minimum of "
                         f"{MIN_SIZE[net_type]}x{MIN_SIZE[net_type]}")
    taps = trunk_features_host(torch.stack([x, y.to(device=x.device, dtype=x.dtype)]), weights)
    lin = weights.to(x.device, x.dtype).lin
    res = [head_host(t[0:1], t[1:2], lin[k]) for k, t in enumerate(taps)]
    return torch.sum(torch.cat(res, 0), 0, True)
