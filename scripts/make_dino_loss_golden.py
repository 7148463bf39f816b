"""Captures tests/golden/dino_loss.npz from the reference's own utils.loss_utils.dino_loss:

    python scripts/make_dino_loss_golden.py /path/to/reference [tests/golden/dino_loss.npz]

The encoder is a stub that hands back given fp16 embeddings (the reference's encoder returns fp16), so the file holds only
the embedding pairs, the lambdas and the reference's fp16 results (stored as their fp32 values); no network and no weights
are involved.  Pairs: random ones of several widths, a pair with a negative cosine at lambda 0.05 (fp16(0.05) != 0.05 and
the product is not -0.05 x cos either), a nearly parallel and a weakly correlated pair.  Every value stays in fp16's normal
range (|value| >= 2^-14), where one rounding is the relative 2^-11 the test's bar assumes."""
import os
import sys

import numpy as np
import torch


class Stub:
    def __init__(self, a, b):
        self.queue = [a, b]

    def encode_tensor(self, image):
        return self.queue.pop(0)


def main():
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                             "tests", "golden", "dino_loss.npz")
    sys.path.insert(0, ref)
    from utils.loss_utils import dino_loss
    g = torch.Generator().manual_seed(2024)
    cases = []
    for n, lam in ((768, 0.05), (384, 0.05), (128, 0.1), (1024, 0.013), (768, 1.0)):
        a = torch.randn(n, generator=g)
        cases.append((a, 0.6 * a + 0.8 * torch.randn(n, generator=g), lam))
    a = torch.randn(768, generator=g)
    cases.append((a, -0.7 * a + 0.5 * torch.randn(768, generator=g), 0.05))       # cosine below 0
    cases.append((a, a + 0.01 * torch.randn(768, generator=g), 0.05))             # nearly parallel
    b = torch.randn(768, generator=g)
    cases.append((a, 0.05 * a + b, 0.05))                                         # weakly correlated: cosine near 0.05
    store = {"n_cases": np.int64(len(cases))}
    img = torch.zeros(3, 16, 16)
    for i, (a, b, lam) in enumerate(cases):
        a16, b16 = (5.0 * a).to(torch.float16), (5.0 * b).to(torch.float16)
        val = dino_loss(img, img, Stub(a16, b16), lam)
        assert val.dtype == torch.float16 and val.dim() == 0, (val.dtype, val.shape)
        store[f"a{i}"], store[f"b{i}"] = a16.numpy(), b16.numpy()
        store[f"lambda{i}"], store[f"golden{i}"] = np.float64(lam), np.float32(float(val))
    np.savez(out, **store)
    print(f"wrote {out}: {len(cases)} cases")


if __name__ == "__main__":
    main()
