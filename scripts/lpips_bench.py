"""Time LPIPS on one GPU: the kernels of csrc/lpips.hip against the torch / MIOpen formulation of the same layers
(gaussmart_amd.lpips.lpips_host moved to the same device), both nets, at 1600x1200 and 1920x1080.

    python scripts/lpips_bench.py [--out profiles/lpips_bench.txt] [--sizes 1600x1200,1920x1080] [--nets vgg,alex]

Per layer (each convolution with its bias and relu, each pool, each head) both sides get the SAME input -- the torch trunk's
activation in front of that layer -- and the table gives best-of-three milliseconds after one warm-up call, with a device
synchronisation behind every timed call, the layer's useful FLOP (2 K per output element) and the rate the kernel reached.
The whole distance follows: the kernel path (gsr_lpips_forward: workspace allocation and every launch) against lpips_host,
with the peak device memory of either beyond the weights and the two images.  The two results are printed side by side and
the run stops if they differ by more than 1e-4 relative (a sanity stop; the tests hold the kernels to the fp64 twin).  Reads nothing outside the repository: weights and images are seeded random.

The torch side: MIOpen's user database lives in a scratch directory of this run (removed at exit), so it starts empty.  By
default torch.backends.cudnn.benchmark is on, i.e. every convolution shape goes through MIOpen's find in the warm-up call and
the timed calls run the solver it picked -- the strongest torch side available here; --no-find times torch's default
(immediate mode: MIOpen's heuristic choice without a find), which is what a script that sets nothing gets.  The header line
of the output says which.
"""
import argparse
import atexit
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# MIOpen writes its find results beside the user's home by default; keep them in a scratch directory of this run
if "MIOPEN_USER_DB_PATH" not in os.environ:
    os.environ["MIOPEN_USER_DB_PATH"] = tempfile.mkdtemp(prefix="miopen_db_")
    atexit.register(shutil.rmtree, os.environ["MIOPEN_USER_DB_PATH"], True)
os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.environ["MIOPEN_USER_DB_PATH"])

import torch                      # noqa: E402
import torch.nn.functional as F   # noqa: E402

from gaussmart_amd import _lib, lpips as LP                  # noqa: E402
from gaussmart_amd._dev import ptr, stream, workspace       # noqa: E402


def best_of(fn, dev, n=3):
    fn()
    torch.cuda.synchronize(dev)
    best = float("inf")
    for _ in range(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def conv_kernel(x, w, b, stride, pad, zscore, y):
    B, ci, H, W = x.shape
    co, _, k, _ = w.shape
    _lib.check(_lib.lib().gsr_lpips_conv(ptr(x), ptr(w), ptr(b), B, ci, H, W, co, k, stride, pad, zscore, ptr(y), stream(x.device)))


def pool_kernel(x, k, y):
    B, c, H, W = x.shape
    _lib.check(_lib.lib().gsr_lpips_pool(ptr(x), B * c, H, W, k, ptr(y), stream(x.device)))


def head_kernel(feat, lin, ws, out):
    _, c, H, W = feat.shape
    _lib.check(_lib.lib().gsr_lpips_head(ptr(feat), ptr(lin), c, H, W, ptr(ws), ws.numel(), ptr(out), stream(feat.device)))


def layer_table(net_type, H, W, weights, dev, say):
    w = weights.to(dev, torch.float32)
    g = torch.Generator().manual_seed(H + W)
    x = torch.rand(2, 3, H, W, generator=g).to(dev)
    mean = torch.tensor(LP.Z_MEAN, device=dev)[None, :, None, None]
    std = torch.tensor(LP.Z_STD, device=dev)[None, :, None, None]
    head_ws = workspace(_lib.lib().gsr_lpips_head_workspace_bytes(), dev)
    head_out = torch.empty(1, device=dev)
    say(f"  {'layer':<28}{'output':>16}{'GFLOP':>9}{'kernel ms':>11}{'TFLOP/s':>9}{'torch ms':>10}{'kernel/torch':>14}")
    tot_k = tot_t = 0.0
    tap = 0
    for l, (ci, co, k, stride, pad, pool, tapped) in enumerate(LP.TRUNK[net_type]):
        rows = []
        if pool:
            y = torch.empty(2, ci, (x.shape[2] - pool) // 2 + 1, (x.shape[3] - pool) // 2 + 1, device=dev)
            tk = best_of(lambda: pool_kernel(x, pool, y), dev)
            tt = best_of(lambda: F.max_pool2d(x, kernel_size=pool, stride=2), dev)
            rows.append((f"pool {pool}x{pool} s2 ({ci})", y.shape, 0.0, tk, tt))
            x = F.max_pool2d(x, kernel_size=pool, stride=2)
            del y
        oh, ow = (x.shape[2] + 2 * pad - k) // stride + 1, (x.shape[3] + 2 * pad - k) // stride + 1
        y = torch.empty(2, co, oh, ow, device=dev)
        gflop = 2.0 * ci * k * k * y.numel() / 1e9
        if l == 0:
            torch_fn = lambda: F.relu_(F.conv2d((x - mean) / std, w.conv_w[l], w.conv_b[l], stride=stride, padding=pad))
        else:
            torch_fn = lambda: F.relu_(F.conv2d(x, w.conv_w[l], w.conv_b[l], stride=stride, padding=pad))
        tk = best_of(lambda: conv_kernel(x, w.conv_w[l], w.conv_b[l], stride, pad, int(l == 0), y), dev)
        tt = best_of(torch_fn, dev)
        rows.append((f"conv{l} {ci}->{co} k{k} s{stride} +relu" + (" +z" if l == 0 else ""), y.shape, gflop, tk, tt))
        del y
        x = torch_fn()
        if tapped:
            tk = best_of(lambda: head_kernel(x, w.lin[tap], head_ws, head_out), dev)
            tt = best_of(lambda: LP.head_host(x[0:1], x[1:2], w.lin[tap]), dev)
            rows.append((f"head {tap} ({co})", x.shape, 0.0, tk, tt))
            tap += 1
        for name, shape, gf, tk, tt in rows:
            rate = f"{gf / tk:9.1f}" if gf else f"{'':>9}"
            say(f"  {name:<28}{'x'.join(map(str, shape[1:])):>16}{gf:9.1f}{tk:11.3f}{rate}{tt:10.3f}{tk / tt:14.2f}")
            tot_k += tk
            tot_t += tt
    say(f"  {'sum of the layers':<28}{'':>16}{'':>9}{tot_k:11.3f}{'':>9}{tot_t:10.3f}{tot_k / tot_t:14.2f}")


def whole(net_type, H, W, weights, dev, say):
    g = torch.Generator().manual_seed(H * 3 + W)
    a = torch.rand(3, H, W, generator=g)
    b = (a + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    a, b = a.to(dev), b.to(dev)
    crit = LP.LPIPS(net_type=net_type, weights=weights)
    wdev = weights.to(dev, torch.float32)
    res = {}
    for name, fn in (("kernels", lambda: crit(a, b)), ("torch", lambda: LP.lpips_host(a, b, net_type=net_type, weights=wdev))):
        fn()
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ms = best_of(fn, dev)
        res[name] = (ms, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, float(fn()))
    (tk, mk, vk), (tt, mt, vt) = res["kernels"], res["torch"]
    say(f"  whole distance: kernels {tk:.3f} ms, peak {mk:.0f} MiB beyond weights and images; torch {tt:.3f} ms, peak {mt:.0f} MiB; "
        f"kernel/torch time {tk / tt:.2f}, memory {mk / max(mt, 1e-9):.2f}")
    say(f"  values: kernels {vk:.8e}, torch {vt:.8e}, relative difference {abs(vk - vt) / abs(vt):.2e}")
    # a sanity stop, not a test (tests/test_gpu_lpips.py holds the kernels to the fp64 twin): the solver MIOpen's find picks
    # for the torch side may be a transform-domain one whose own error is above the fp32 summation level
    if not abs(vk - vt) <= 1e-4 * abs(vt):
        raise SystemExit(f"lpips_bench: the two paths disagree: {vk} vs {vt}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.txt"))
    ap.add_argument("--sizes", default="1600x1200,1920x1080")
    ap.add_argument("--nets", default="vgg,alex")
    ap.add_argument("--no-find", action="store_true", help="torch's default (MIOpen immediate mode) instead of its find")
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = not args.no_find
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench: no GPU (a timing needs the device)")
    dev = torch.device("cuda", 0)
    _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"LPIPS, kernels (csrc/lpips.hip) against the torch formulation on {torch.cuda.get_device_name(dev)}; fp32, batch of 2 "
        "(the pair); best of 3 after a warm-up, host clock around a synchronised call; seeded random weights and images; torch side: "
        + ("MIOpen immediate mode (torch's default), empty user database" if args.no_find else
           "MIOpen find in the warm-up call (torch.backends.cudnn.benchmark), user database empty at the start"))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for net_type in args.nets.split(","):
            weights = LP.random_lpips_weights(net_type, seed=1)
            say("")
            say(f"{net_type} at {W}x{H}")
            layer_table(net_type, H, W, weights, dev, say)
            torch.cuda.empty_cache()
            whole(net_type, H, W, weights, dev, say)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
