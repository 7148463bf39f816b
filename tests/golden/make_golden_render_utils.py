"""Regenerate tests/golden/render_utils.npz: focus_point_fn and the bounding radius of GaussianExtractor.
estimate_bounding_sphere (utils/mesh_utils.py:114-124) computed by the reference's own utils/render_utils.py on the CPU.

    python tests/golden/make_golden_render_utils.py /path/to/reference/checkout

mediapy (imported at the top of render_utils.py, used only for videos) is stubbed in sys.modules."""
import os
import sys
import types

import numpy as np


def main(ref_root):
    sys.modules.setdefault("mediapy", types.ModuleType("mediapy"))
    sys.path.insert(0, ref_root)
    from utils.render_utils import focus_point_fn
    rng = np.random.default_rng(5)
    cases = {}
    for k, n in enumerate((3, 8, 49)):
        # cameras on a noisy sphere looking roughly at a point near the origin
        eye = rng.normal(size=(n, 3))
        eye = eye / np.linalg.norm(eye, axis=1, keepdims=True) * (2.0 + rng.uniform(0, 1, (n, 1)))
        target = rng.normal(scale=0.1, size=3)
        c2ws = np.zeros((n, 4, 4))
        for i in range(n):
            fwd = target - eye[i] + rng.normal(scale=0.02, size=3)
            fwd /= np.linalg.norm(fwd)
            right = np.cross(fwd, [0.0, 0.0, 1.0])
            right /= np.linalg.norm(right)
            down = np.cross(fwd, right)
            c2ws[i, :3, :3] = np.stack([right, down, fwd], 1)
            c2ws[i, :3, 3] = eye[i]
            c2ws[i, 3, 3] = 1
        poses = c2ws[:, :3, :] @ np.diag([1, -1, -1, 1])
        center = focus_point_fn(poses)
        radius = np.linalg.norm(c2ws[:, :3, 3] - center, axis=-1).min()
        cases[f"c2ws_{k}"] = c2ws
        cases[f"center_{k}"] = center
        cases[f"radius_{k}"] = np.float64(radius)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render_utils.npz")
    np.savez(out, **cases)
    print(f"wrote {out}")


if __name__ == "__main__":
    main(sys.argv[1])
