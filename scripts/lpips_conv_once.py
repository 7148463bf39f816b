"""Developer aid for counter passes (rocprofv3 --kernel-trace --pmc ... -- python scripts/lpips_conv_once.py): three of VGG16's
convolutions at the 1600x1200 sizes through gsr_lpips_conv, two launches each after one warm-up, seeded random data."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussmart_amd import _lib                          # noqa: E402
from gaussmart_amd._dev import ptr, stream              # noqa: E402

LAYERS = ((64, 64, 1200, 1600), (256, 256, 300, 400), (512, 512, 150, 200))


def main():
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    for ci, co, H, W in LAYERS:
        x = torch.rand(2, ci, H, W, generator=g).to(dev)
        w = (torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5).to(dev)
        b = (0.05 * torch.randn(co, generator=g)).to(dev)
        y = torch.empty(2, co, H, W, device=dev)
        for _ in range(3):
            _lib.check(_lib.lib().gsr_lpips_conv(ptr(x), ptr(w), ptr(b), 2, ci, H, W, co, 3, 1, 1, 0, ptr(y), stream(dev)))
        torch.cuda.synchronize(dev)
        print(ci, co, H, W, float(y.mean()))


if __name__ == "__main__":
    main()
