"""Regenerate tests/golden/mcubes.npz: scikit-image's marching_cubes(method="lorensen") on four small fields, the independent
pin of gaussmart_amd/csrc/mcubes.hip (tests/test_gpu_mesh.py).  Needs scikit-image (0.18 was used):

    python tests/golden/make_golden_mcubes.py          # with an interpreter that imports skimage

Stored per field NAME: NAME_field f32 [X,Y,Z], NAME_verts f32 [V,3] (index coordinates, level 0), NAME_faces i32 [F,3], and
NAME_ambiguous (number of cube faces whose four signs alternate).  The generator asserts that the sphere, the torus and the
two touching spheres have no ambiguous face and that the noisy field has some.
"""
import os

import numpy as np


def fields():
    n = 40
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    c = (n - 1) / 2
    out = {}
    out["sphere"] = (np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 12.3) / 5
    q = np.sqrt((x - c) ** 2 + (y - c) ** 2) - 11.0
    out["torus"] = (np.sqrt(q ** 2 + (z - c) ** 2) - 4.6) / 5
    s1 = np.sqrt((x - 13.2) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 7.0
    s2 = np.sqrt((x - 27.2) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 7.0
    out["two_spheres"] = np.minimum(s1, s2) / 5
    rng = np.random.default_rng(3)
    noisy = rng.normal(size=(24, 24, 24)) + 0.3
    noisy[[0, -1]] = noisy[:, [0, -1]] = noisy[:, :, [0, -1]] = 1.0
    out["noisy"] = noisy
    return {k: v.astype(np.float32) for k, v in out.items()}


def ambiguous_faces(f):
    """Cube faces (shared ones counted once) whose corners, walked around the face, alternate in sign (tsdf < 0)."""
    neg = f < 0
    count = 0
    for a in range(3):
        u, w = [b for b in range(3) if b != a]
        s = [slice(None)] * 3
        def sl(du, dw):
            t = list(s)
            t[u] = slice(du, neg.shape[u] - 1 + du)
            t[w] = slice(dw, neg.shape[w] - 1 + dw)
            return neg[tuple(t)]
        p00, p10, p11, p01 = sl(0, 0), sl(1, 0), sl(1, 1), sl(0, 1)
        count += int(((p00 == p11) & (p10 == p01) & (p00 != p10)).sum())
    return count


def main():
    from skimage.measure import marching_cubes
    out = {}
    for name, f in fields().items():
        verts, faces, _, _ = marching_cubes(f, level=0.0, method="lorensen", allow_degenerate=True)
        amb = ambiguous_faces(f)
        out[f"{name}_field"] = f
        out[f"{name}_verts"] = verts.astype(np.float32)
        out[f"{name}_faces"] = faces.astype(np.int32)
        out[f"{name}_ambiguous"] = np.int64(amb)
        print(f"{name}: {len(verts)} vertices, {len(faces)} triangles, {amb} ambiguous faces")
    for name in ("sphere", "torus", "two_spheres"):
        assert out[f"{name}_ambiguous"] == 0, f"{name} has ambiguous faces"
    assert out["noisy_ambiguous"] > 0, "the noisy field has no ambiguous face"
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mcubes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
