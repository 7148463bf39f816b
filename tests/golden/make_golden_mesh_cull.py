"""Writes mesh_cull_dilate.npz beside this file: scipy.ndimage.binary_dilation (disk dx^2 + dy^2 <= r^2) of the dilation test
images (tests/mesh_cull_ref.py: dilation_images) for the (size, radius) cases that take scipy too long to run inside the
test suite -- minutes in all.  Bit-packed results plus a CRC of the input images.

    python tests/golden/make_golden_mesh_cull.py
"""
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import mesh_cull_ref as R
    out = {}
    for H, W in R.DILATE_SIZES:
        for r in R.DILATE_RADII:
            if R.dilation_case_is_live(H, W, r):
                continue
            t0 = time.time()
            imgs = R.dilation_images(H, W)
            name = f"{H}x{W}_r{r}"
            out[name] = np.packbits(R.dilate_ref(imgs, r))
            out[name + "_input_crc"] = np.uint32(zlib.crc32(imgs.tobytes()))
            print(f"{name}: {time.time() - t0:.1f} s", flush=True)
    os.makedirs(os.path.dirname(R.DILATE_GOLDEN), exist_ok=True)
    np.savez_compressed(R.DILATE_GOLDEN, **out)
    print(f"wrote {R.DILATE_GOLDEN} ({os.path.getsize(R.DILATE_GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
