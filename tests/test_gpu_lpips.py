"""The LPIPS kernels (csrc/lpips.hip; include/gsr.h: LP_CONV, LP_POOL, LP_HEAD, LP_FORWARD) on the device: each layer
primitive against torch in fp64 on the CPU, the whole distance against the fp64 twin, the refusals, and metrics_cli against
its --host path.  Inputs, the twin's cached values and the tolerance rule are in tests/lpips_cases.py (a golden vector of the
reference cannot exist: its LPIPS package needs torchvision and the network)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import lpips_cases as LC
from gaussmart_amd import _lib
from gaussmart_amd import lpips as LP
from gaussmart_amd._dev import ptr, stream, workspace

pytestmark = pytest.mark.gpu


def conv_dev(x, w, b, stride, pad, zscore=0):
    B, ci, H, W = x.shape
    co, _, k, _ = w.shape
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.full((B, co, oh, ow), float("nan"), device=x.device)
    _lib.check(_lib.lib().gsr_lpips_conv(ptr(x), ptr(w), ptr(b), B, ci, H, W, co, k, stride, pad, zscore, ptr(y), stream(x.device)))
    return y


def pool_dev(x, k):
    B, c, H, W = x.shape
    y = torch.full((B, c, (H - k) // 2 + 1, (W - k) // 2 + 1), float("nan"), device=x.device)
    _lib.check(_lib.lib().gsr_lpips_pool(ptr(x), B * c, H, W, k, ptr(y), stream(x.device)))
    return y


def head_dev(feat, lin):
    _, c, H, W = feat.shape
    L = _lib.lib()
    nbytes = L.gsr_lpips_head_workspace_bytes()
    ws = workspace(nbytes, feat.device)
    out = torch.full((1,), float("nan"), device=feat.device)
    _lib.check(L.gsr_lpips_head(ptr(feat), ptr(lin), c, H, W, ptr(ws), nbytes, ptr(out), stream(feat.device)))
    return float(out)


CONVS = {"3-64-k3": (3, 64, 3, 1, 1), "64-128-k3": (64, 128, 3, 1, 1), "192-384-k3": (192, 384, 3, 1, 1),
         "3-64-k11s4": (3, 64, 11, 4, 2), "64-192-k5": (64, 192, 5, 1, 2)}
# 7x309: wide enough that some tiles of 128 / 256 consecutive pixels have every window inside the image (the kernel's path
# without bounds comparisons) next to ragged ones; the four small planes only ever take the checked path
PLANES = [(1, 1), (7, 5), (33, 65), (16, 130), (7, 309)]


def inside_tiles(B, plane, H, W, k, s, p, c_out):
    """How many workgroups of a launch take the convolution's `inside` path: the kernel's own decision restated (a tile of
    128 pixels where C_out is a multiple of 128, else 256; flattened (b, oy, ox) order)."""
    oh, ow = plane
    bn = 128 if c_out % 128 == 0 else 256
    npix, n = B * oh * ow, 0
    for t in range(npix // bn):
        q = torch.arange(t * bn, (t + 1) * bn) % (oh * ow)
        iy, ix = (q // ow) * s - p, (q % ow) * s - p
        n += bool(((iy >= 0) & (ix >= 0) & (iy + k <= H) & (ix + k <= W)).all())
    return n


def _conv_inputs(cfg, plane, seed=0):
    ci, co, k, s, p = CONVS[cfg]
    oh, ow = plane
    H, W = (oh - 1) * s + k - 2 * p, (ow - 1) * s + k - 2 * p
    g = torch.Generator().manual_seed(seed + 7 * oh + ow + ci)
    x = torch.rand(2, ci, H, W, generator=g) * 2 - 0.5
    w = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    b = 0.05 * torch.randn(co, generator=g)
    return x, w, b, s, p


def _conv_bound(x, w, b, s, p):
    """fp64 reference of relu(conv) and the derived bound gamma_K (|w| * |x|) + 2^-23 |out|, K = C_in k^2: it holds for any
    order of the K products' summation."""
    K = w[0].numel()
    u = K * 2.0 ** -24
    gamma = u / (1 - u)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p))
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride=s, padding=p)
    return ref, gamma * mag + 2.0 ** -23 * ref.abs()


@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("cfg", list(CONVS))
def test_conv_against_fp64(gpu_device, cfg, plane):
    x, w, b, s, p = _conv_inputs(cfg, plane)
    ref, bound = _conv_bound(x, w, b, s, p)
    got = conv_dev(x.to(gpu_device), w.to(gpu_device), b.to(gpu_device), s, p).cpu().double()
    assert got.shape == ref.shape == (2, CONVS[cfg][1]) + plane
    err = (got - ref).abs()
    print(f"{cfg} {plane}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert torch.isfinite(got).all() and bool((err <= bound).all())
    ci, co, k = CONVS[cfg][:3]
    n_inside = inside_tiles(2, plane, x.shape[2], x.shape[3], k, s, p, co)
    assert (n_inside >= 2) == (plane == (7, 309)), (cfg, plane, n_inside)      # both gather paths are covered, knowingly
    # the two images of the batch run through one launch; each alone (another tiling) gives the same bits
    one = conv_dev(x[1:].to(gpu_device), w.to(gpu_device), b.to(gpu_device), s, p).cpu().double()
    assert torch.equal(one[0], got[1])
    if ci == 3:
        # the z-score in the load: fp32 (x - mean) / std as the kernel forms it, then F.conv2d's zero padding
        mean = torch.tensor(LP.Z_MEAN, dtype=torch.float32)[None, :, None, None]
        std = torch.tensor(LP.Z_STD, dtype=torch.float32)[None, :, None, None]
        ref, bound = _conv_bound((x - mean) / std, w, b, s, p)
        got = conv_dev(x.to(gpu_device), w.to(gpu_device), b.to(gpu_device), s, p, zscore=1).cpu().double()
        assert torch.isfinite(got).all() and bool(((got - ref).abs() <= bound).all())


@pytest.mark.parametrize("cfg", list(CONVS))
def test_conv_where_only_zeros_are_seen_is_relu_bias(gpu_device, cfg):
    """An output whose whole receptive field is padding and zeros is exactly relu(bias); with zscore the padding stays 0 after
    the normalisation while the image's own zeros become (0 - mean) / std."""
    ci, co, k, s, p = CONVS[cfg]
    H = W = 4 * k + 9 if s == 1 else 75
    g = torch.Generator().manual_seed(11)
    x = torch.zeros(2, ci, H, W)
    y0 = H // 2 + k                                    # only the far corner carries values
    x[:, :, y0:, y0:] = torch.rand(2, ci, H - y0, W - y0, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    b = 0.05 * torch.randn(co, generator=g)
    got = conv_dev(x.to(gpu_device), w.to(gpu_device), b.to(gpu_device), s, p).cpu()
    n = (y0 + p - k) // s + 1                           # outputs [0, n) read rows / columns up to (n-1) s - p + k - 1 < y0
    assert n >= 2
    want = F.relu(b)[None, :, None, None].expand(2, co, n, n)
    assert torch.equal(got[:, :, :n, :n], want)
    ref, bound = _conv_bound(x, w, b, s, p)
    assert bool(((got.double() - ref).abs() <= bound).all())
    if ci == 3:
        mean = torch.tensor(LP.Z_MEAN, dtype=torch.float32)[None, :, None, None]
        std = torch.tensor(LP.Z_STD, dtype=torch.float32)[None, :, None, None]
        z = (x - mean) / std                            # fp32, as the kernel forms it; F.conv2d then pads with zeros
        ref, bound = _conv_bound(z, w, b, s, p)
        got = conv_dev(x.to(gpu_device), w.to(gpu_device), b.to(gpu_device), s, p, zscore=1).cpu().double()
        assert bool(((got - ref).abs() <= bound).all())


@pytest.mark.parametrize("k", [2, 3])
def test_pool_is_bit_equal(gpu_device, k):
    g = torch.Generator().manual_seed(2)
    for H in (2, 3, 7, 8, 33):
        for W in (2, 3, 7, 8, 33):
            if H < k or W < k:
                continue
            x = torch.randn(2, 5, H, W, generator=g)
            x[0, 0, 0, 0] = float("-inf")
            assert torch.equal(pool_dev(x.to(gpu_device), k).cpu(), F.max_pool2d(x, kernel_size=k, stride=2)), (k, H, W)


@pytest.mark.parametrize("C,H,W", [(64, 7, 5), (192, 33, 65), (512, 16, 130), (40, 9, 11), (64, 200, 180)])
def test_head_against_fp64_twin(gpu_device, C, H, W):
    g = torch.Generator().manual_seed(C + H)
    feat = F.relu(torch.randn(2, C, H, W, generator=g) + 0.3)
    feat[0, :, 0, 0] = 0.0              # all channels zero in one image
    feat[:, :, H - 1, W - 1] = 0.0      # and in both
    feat[1, :, H // 2, W // 2] = 0.0
    lin = torch.rand(C, generator=g) / C
    v64 = float(LP.head_host(feat[0:1].double(), feat[1:2].double(), lin.double()))
    v32 = float(LP.head_host(feat[0:1], feat[1:2], lin))
    tol = 4.0 * max(abs(v32 - v64), 2.0 ** -23 * abs(v64))
    got = head_dev(feat.to(gpu_device), lin.to(gpu_device))
    print(f"head C {C} {H}x{W}: value {v64:.8e}, device off by {abs(got - v64):.2e}, fp32 twin by {abs(v32 - v64):.2e}, bar {tol:.2e}")
    assert got == got and abs(got) != float("inf")
    assert abs(got - v64) <= tol
    same = feat.clone()
    same[1] = same[0]
    assert head_dev(same.to(gpu_device), lin.to(gpu_device)) == 0.0


E2E = [("vgg", 16, 16), ("alex", 31, 31), ("vgg", 35, 67), ("alex", 35, 67), ("vgg", 64, 48), ("alex", 64, 48), ("vgg", 193, 257),
       # wide enough for tiles on the convolution's `inside` path, z-score included: VGG's first four layers, AlexNet's first
       ("vgg", 20, 300), ("alex", 80, 1200)]


@pytest.mark.parametrize("net_type,H,W", E2E)
def test_end_to_end_against_fp64_twin(gpu_device, net_type, H, W):
    w = LC.weights(net_type)
    x, y = (t.to(gpu_device) for t in LC.image_pair(H, W))
    crit = LP.LPIPS(net_type=net_type, weights=w)
    got = crit(x, y)
    assert got.shape == (1, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
    v64, tol = LC.twin(net_type, H, W, torch.float64), LC.tolerance(net_type, H, W)
    print(f"{net_type} {H}x{W}: value {v64:.8e}, device off by {abs(float(got) - v64):.2e}, "
          f"fp32 twin by {abs(LC.twin(net_type, H, W, torch.float32) - v64):.2e}, bar {tol:.2e}")
    assert abs(float(got) - v64) <= tol
    assert float(crit(x, x)) == 0.0                                  # identical images
    assert torch.equal(crit(x, y), got)                              # the same bits on every run
    assert abs(float(crit(y, x)) - v64) <= tol                       # symmetric
    assert torch.equal(LP.lpips(x[None], y[None], net_type=net_type, weights=w), got)       # the function, [1,3,H,W]


def test_value_range_is_passed_through_on_the_device(gpu_device):
    w = LC.weights("alex")
    x, y = LC.image_pair(35, 67)
    want = float(LP.lpips_host((x * 2 - 1).double(), (y * 2 - 1).double(), net_type="alex", weights=w))
    want32 = float(LP.lpips_host(x * 2 - 1, y * 2 - 1, net_type="alex", weights=w))
    got = float(LP.lpips((x * 2 - 1).to(gpu_device), (y * 2 - 1).to(gpu_device), net_type="alex", weights=w))
    assert abs(got - want) <= 4.0 * max(abs(want32 - want), 2.0 ** -23 * abs(want))


def test_refusals(gpu_device):
    dev = gpu_device
    wv, wa = LC.weights("vgg"), LC.weights("alex")
    with pytest.raises(_lib.GsrError, match="below the vgg"):
        LP.lpips(torch.rand(3, 15, 15, device=dev), torch.rand(3, 15, 15, device=dev), net_type="vgg", weights=wv)
    with pytest.raises(_lib.GsrError, match="below the alex"):
        LP.lpips(torch.rand(3, 30, 40, device=dev), torch.rand(3, 30, 40, device=dev), net_type="alex", weights=wa)
    with pytest.raises(ValueError, match="batch of 2"):
        LP.lpips(torch.rand(2, 3, 32, 32, device=dev), torch.rand(2, 3, 32, 32, device=dev), net_type="alex", weights=wa)
    with pytest.raises(_lib.GsrError, match="3 channels"):
        LP.lpips(torch.rand(4, 32, 32, device=dev), torch.rand(4, 32, 32, device=dev), net_type="alex", weights=wa)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        LP.lpips(torch.rand(3, 32, 32), torch.rand(3, 32, 32), net_type="alex", weights=wa)
    with pytest.raises(NotImplementedError, match="squeeze"):
        LP.lpips(torch.rand(3, 32, 32, device=dev), torch.rand(3, 32, 32, device=dev), net_type="squeeze", weights=wa)
    # the primitives refuse what they do not implement, before anything is launched
    L = _lib.lib()
    x = torch.rand(2, 3, 8, 8, device=dev)
    null = ptr(None)
    assert L.gsr_lpips_conv(ptr(x), null, ptr(x), 2, 3, 8, 8, 64, 3, 1, 1, 0, ptr(x), stream(dev)) == -1      # null weights
    assert L.gsr_lpips_conv(ptr(x), ptr(x), ptr(x), 2, 3, 8, 8, 64, 7, 1, 1, 0, ptr(x), stream(dev)) == -4     # kernel size 7
    assert L.gsr_lpips_pool(ptr(x), 6, 2, 8, 3, ptr(x), stream(dev)) == -1                                     # plane < window
    assert L.gsr_lpips_head(ptr(x), ptr(x), 3, 8, 8, ptr(x), 4096, ptr(x), stream(dev)) == -4                  # C = 3
    assert L.gsr_lpips_workspace_bytes(7, 32, 32) == 0


def test_metrics_cli_device_against_host(gpu_device, tmp_path):
    from gaussmart_amd import metrics_cli
    wdir = tmp_path / "w"
    wdir.mkdir()
    LC.write_weight_files(wdir, "alex")
    out = {}
    for mode in ("host", "device"):
        model = str(tmp_path / mode)
        names = LC.write_model(model)
        argv = ["-m", model, "--lpips_dir", str(wdir), "--lpips_net", "alex"] + (["--host"] if mode == "host" else [])
        assert metrics_cli.main(argv) == 0
        out[mode] = (json.load(open(os.path.join(model, "results.json"))), json.load(open(os.path.join(model, "per_view.json"))))
    w = LC.weights("alex")
    for n in names:
        h, d = out["host"][1]["ours_30000"], out["device"][1]["ours_30000"]
        assert abs(d["SSIM"][n] - h["SSIM"][n]) < 2e-6
        assert abs(d["PSNR"][n] - h["PSNR"][n]) < 1e-5 * abs(h["PSNR"][n])
        r, g = LC.load_pair(str(tmp_path / "host"), "ours_30000", n)
        v64 = float(LP.lpips_host(r.double(), g.double(), net_type="alex", weights=w))
        tol = 4.0 * max(abs(h["LPIPS"][n] - v64), 2.0 ** -23 * abs(v64))
        assert abs(d["LPIPS"][n] - v64) <= tol, (n, d["LPIPS"][n], v64, tol)
    assert list(out["device"][1]["ours_30000"]["LPIPS"]) == names
    assert abs(out["device"][0]["ours_30000"]["SSIM"] - out["host"][0]["ours_30000"]["SSIM"]) < 2e-6
    assert out["device"][0]["ours_30000"]["LPIPS"] is not None
