#!/usr/bin/env python3
"""Byte-compare two `bench.py --dump-outputs` directories (two builds, same arguments): every array of the manifest must
exist in both and hold the same bytes.  Usage: python3 scripts/compare_dumps.py DIR_A DIR_B   (exit status 1 on a difference)"""
import json
import os
import sys

import numpy as np


def main(a, b):
    ma, mb = (json.load(open(os.path.join(d, "manifest.json"))) for d in (a, b))
    names = sorted(set(ma) | set(mb))
    bad = 0
    for n in names:
        fa, fb = os.path.join(a, n + ".npy"), os.path.join(b, n + ".npy")
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print(f"{n}: missing in {'A' if not os.path.exists(fa) else 'B'}"); bad += 1
            continue
        xa, xb = np.load(fa), np.load(fb)
        same = xa.shape == xb.shape and xa.dtype == xb.dtype and xa.tobytes() == xb.tobytes()
        if not same:
            diff = int((xa != xb).sum()) if xa.shape == xb.shape else -1
            print(f"{n}: DIFFERENT ({diff} of {xa.size} elements)"); bad += 1
    print(f"{len(names)} arrays, {bad} different: {a} vs {b}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
