"""SSIM, PSNR and LPIPS of rendered test views: the reference's metrics.py (metrics.py:36-92), the third step of every
evaluation script after training and render_cli.

    python -m gaussmart_amd.metrics_cli -m MODEL [MODEL ...] [--lpips_dir DIR] [--lpips_net vgg] [--host]

For every MODEL/test/<method>/{renders,gt} the PNGs are paired by name (sorted; the reference takes os.listdir order), the
first three channels divided by 255, and MODEL/results.json and MODEL/per_view.json are written with the reference's keys
and nesting.  SSIM is loss_utils.ssim (the fused kernel), PSNR is utils/image_utils.py:19-21, LPIPS is gaussmart_amd.lpips
with the weights of --lpips_dir (vgg: vgg16.pth + vgg.pth; alex: alexnet.pth + alex.pth; nothing is downloaded).  Without
--lpips_dir the LPIPS entries are null.  --host runs the torch formulations on the CPU instead of the kernels.  Images are
uploaded once and stay on the device.  A scene that fails is reported with its error and the others still run; the exit
status is then 1.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import _lib
from . import losses


def read_images(renders_dir, gt_dir, device):
    from PIL import Image
    renders, gts, names = [], [], []
    for fname in sorted(os.listdir(renders_dir)):
        pair = []
        for d in (renders_dir, gt_dir):
            a = np.array(Image.open(os.path.join(d, fname)))
            if a.ndim == 2:
                a = a[:, :, None]
            t = torch.from_numpy(a).permute(2, 0, 1)[:3].to(device)
            pair.append((t.to(torch.float32) / 255.0).unsqueeze(0).contiguous())
        renders.append(pair[0])
        gts.append(pair[1])
        names.append(fname)
    return renders, gts, names


def _mean(values):
    return torch.tensor(values).mean().item()


def evaluate_method(method_dir, device, host, lpips_fn):
    """-> (results dict, per-view dict) of one MODEL/test/<method>."""
    renders, gts, names = read_images(os.path.join(method_dir, "renders"), os.path.join(method_dir, "gt"), device)
    if not names:
        raise FileNotFoundError(f"{os.path.join(method_dir, 'renders')}: no images")
    if host:
        ssim_fn = losses.ssim
    else:
        from .loss_utils import ssim as ssim_fn
    ssims, psnrs, lpipss = [], [], []
    for r, g in zip(renders, gts):
        ssims.append(float(ssim_fn(r, g)))
        psnrs.append(float(losses.psnr(r, g)))
        if lpips_fn is not None:
            lpipss.append(float(lpips_fn(r, g)))
    full = {"SSIM": _mean(ssims), "PSNR": _mean(psnrs), "LPIPS": _mean(lpipss) if lpips_fn is not None else None}
    per_view = {"SSIM": dict(zip(names, torch.tensor(ssims).tolist())),
                "PSNR": dict(zip(names, torch.tensor(psnrs).tolist())),
                "LPIPS": dict(zip(names, torch.tensor(lpipss).tolist() if lpips_fn is not None else [None] * len(names)))}
    return full, per_view


def evaluate(model_paths, lpips_dir=None, lpips_net="vgg", host=False):
    """Writes results.json / per_view.json into every model directory; -> {model: error text} of the scenes that failed."""
    device = torch.device("cpu")
    if not host:
        if not torch.cuda.is_available():
            raise _lib.GsrError("no GPU: the device path has no CPU fall-back (use --host)")
        device = torch.device("cuda", 0)
    lpips_fn = None
    if lpips_dir:
        from . import lpips as LP
        weights = LP.weights_from_dir(lpips_net, lpips_dir)
        if host:
            lpips_fn = lambda a, b: LP.lpips_host(a, b, net_type=lpips_net, weights=weights)
        else:
            criterion = LP.LPIPS(net_type=lpips_net, weights=weights)
            lpips_fn = criterion
    else:
        print("metrics_cli: no --lpips_dir (the two weight files of LPIPS are local files, nothing is downloaded): LPIPS is null")
    failed = {}
    for scene_dir in model_paths:
        try:
            print("Scene:", scene_dir)
            test_dir = os.path.join(scene_dir, "test")
            full, per_view = {}, {}
            for method in sorted(os.listdir(test_dir)):
                print("Method:", method)
                full[method], per_view[method] = evaluate_method(os.path.join(test_dir, method), device, host, lpips_fn)
                print("  SSIM : {:>12.7f}".format(full[method]["SSIM"]))
                print("  PSNR : {:>12.7f}".format(full[method]["PSNR"]))
                if full[method]["LPIPS"] is not None:
                    print("  LPIPS: {:>12.7f}".format(full[method]["LPIPS"]))
                print("")
            with open(os.path.join(scene_dir, "results.json"), "w") as fp:
                json.dump(full, fp, indent=True)
            with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
                json.dump(per_view, fp, indent=True)
        except (OSError, ValueError, KeyError, RuntimeError) as e:
            failed[scene_dir] = f"{type(e).__name__}: {e}"
            print(f"Unable to compute metrics for model {scene_dir}: {failed[scene_dir]}", file=sys.stderr)
    return failed


def main(argv=None):
    ap = argparse.ArgumentParser(description="SSIM, PSNR and LPIPS of MODEL/test/<method>/{renders,gt}.")
    ap.add_argument("--model_paths", "-m", required=True, nargs="+", type=str, default=[])
    ap.add_argument("--lpips_dir", type=str, default=None, help="directory with the trunk's and the linear layers' weight files")
    ap.add_argument("--lpips_net", type=str, default="vgg", choices=("vgg", "alex"))
    ap.add_argument("--host", action="store_true", help="torch on the CPU instead of the device kernels")
    args = ap.parse_args(argv)
    try:
        failed = evaluate(args.model_paths, args.lpips_dir, args.lpips_net, args.host)
    except (OSError, ValueError, KeyError, NotImplementedError, _lib.GsrError) as e:
        print(f"metrics_cli: {e}", file=sys.stderr)
        return 2
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
