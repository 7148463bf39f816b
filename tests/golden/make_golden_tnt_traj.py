"""Writes tnt_traj.npz beside this file: a dozen random nerfstudio-style camera poses and what the reference's own helper
(scripts/eval_tnt/help_func.py: auto_orient_and_center_poses(method='up', center_poses=True)) followed by get_traj's scaling by
1 / max|t| (scripts/eval_tnt/cull_mesh.py:341-344) makes of them, in torch float32 as the reference runs it.

    python tests/golden/make_golden_tnt_traj.py /path/to/reference/scripts/eval_tnt

gaussmart_amd.mesh_visibility.orient_center_scale restates the same steps in float64; measured difference to this float32
output: 1.4e-7 (largest absolute difference of a matrix entry; the entries are at most 1 in magnitude), which
tests/test_mesh_vis_cpu.py holds to 1e-6 = a few float32 roundings of values up to 6 before the scaling.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def random_poses(n=12, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        m = np.eye(4)
        m[:3, :3] = q
        m[:3, 1] = 0.6 * m[:3, 1] + 0.4 * np.array([0.2, 0.9, 0.3])       # the "up" axes share a direction, as real captures do
        m[:3, 3] = rng.uniform(-4, 6, 3)
        out.append(m)
    return np.stack(out)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import torch
    from help_func import auto_orient_and_center_poses
    c2w = random_poses()
    poses = torch.from_numpy(c2w.astype(np.float32))
    poses, _ = auto_orient_and_center_poses(poses, method="up", center_poses=True)
    poses[:, :3, 3] *= 1.0 / float(torch.max(torch.abs(poses[:, :3, 3])))
    order = np.random.default_rng(3).permutation(len(c2w))                  # the order of the frames in the .json
    path = os.path.join(HERE, "tnt_traj.npz")
    np.savez_compressed(path, c2w_in=c2w, frame_order=order, reference_out=poses.numpy())
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
