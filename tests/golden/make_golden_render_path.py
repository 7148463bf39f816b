"""Regenerate tests/golden/render_path.npz: transform_poses_pca, generate_ellipse_path and the path warped back to the scene
(generate_path's `inv(transform) @ pad_poses(new_poses)`), computed by the reference's own utils/render_utils.py on the CPU
in float64 for three camera sets (n = 3, 12, 49).

    python tests/golden/make_golden_render_path.py /path/to/reference/checkout

mediapy (imported at the top of render_utils.py, used only for videos) is stubbed in sys.modules.  The script asserts that the
sets reach both branches of transform_poses_pca: a negative determinant of the sorted eigenvectors and the y-flip."""
import os
import sys
import types

import numpy as np

SETS = ((3, 0, 1.0), (12, 5, -1.0), (49, 7, 1.0))     # (cameras, seed, sign of the world up-vector the cameras hang from)


def camera_set(n, seed, up_sign):
    """c2w [n,4,4] (COLMAP axes) of cameras on a noisy, flattened sphere looking roughly at a point near the origin."""
    rng = np.random.default_rng(seed)
    eye = rng.normal(size=(n, 3)) * np.array([1.0, 0.7, 0.25])
    eye = eye / np.linalg.norm(eye, axis=1, keepdims=True) * (2.0 + rng.uniform(0, 1, (n, 1)))
    target = rng.normal(scale=0.1, size=3)
    c2ws = np.zeros((n, 4, 4))
    for i in range(n):
        fwd = target - eye[i] + rng.normal(scale=0.02, size=3)
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0.0, 0.0, up_sign])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        c2ws[i, :3, :3] = np.stack([right, down, fwd], 1)
        c2ws[i, :3, 3] = eye[i]
        c2ws[i, 3, 3] = 1
    return c2ws


def branches(poses):
    """(determinant of the sorted eigenvector matrix < 0, y-flip taken) of transform_poses_pca on these poses."""
    t = poses[:, :3, 3] - poses[:, :3, 3].mean(axis=0)
    eigval, eigvec = np.linalg.eig(t.T @ t)
    rot = eigvec[:, np.argsort(eigval)[::-1]].T
    neg = np.linalg.det(rot) < 0
    if neg:
        rot = np.diag(np.array([1, 1, -1])) @ rot
    return bool(neg), bool((rot @ poses[:, :3, :3]).mean(axis=0)[2, 1] < 0)


def main(ref_root):
    sys.modules.setdefault("mediapy", types.ModuleType("mediapy"))
    sys.path.insert(0, ref_root)
    from utils.render_utils import generate_ellipse_path, pad_poses, transform_poses_pca
    cases, seen_neg, seen_flip = {}, set(), set()
    for k, (n, seed, up_sign) in enumerate(SETS):
        c2ws = camera_set(n, seed, up_sign)
        poses = c2ws[:, :3, :] @ np.diag([1, -1, -1, 1])
        neg, flip = branches(poses)
        seen_neg.add(neg)
        seen_flip.add(flip)
        recentered, transform = transform_poses_pca(poses)
        cases[f"c2ws_{k}"] = c2ws
        cases[f"recentered_{k}"] = recentered
        cases[f"transform_{k}"] = transform
        cases[f"branches_{k}"] = np.array([neg, flip])
        for frames in (8, 240):
            path = generate_ellipse_path(poses=recentered, n_frames=frames)
            cases[f"ellipse_{k}_{frames}"] = path
            cases[f"warped_{k}_{frames}"] = np.linalg.inv(transform) @ pad_poses(path)
    assert seen_neg == {False, True}, f"the sets do not reach both determinant signs: {seen_neg}"
    assert seen_flip == {False, True}, f"the sets do not reach both sides of the y-flip: {seen_flip}"
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render_path.npz")
    np.savez(out, **cases)
    print(f"wrote {out}")


if __name__ == "__main__":
    main(sys.argv[1])
