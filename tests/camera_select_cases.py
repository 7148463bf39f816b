"""What the CPU and the GPU tests of the view selection share: the golden file of the reference's CameraClustering
(tests/golden/make_golden_camera_select.py), point sets and initial centres for the Lloyd kernel and its twin, an 8-camera scan
directory as gaussmart_amd.identify_cli, sam_cli and segment_cli read it, and a stub mask generator."""
import functools
import os

import numpy as np

from conftest import GOLDEN
from gaussmart_amd import camera_select as CS
from gaussmart_amd._lib import GSR_CK_KMAX

SETS = ("ring49", "dome64", "dome31", "dome8", "dome7", "blob120", "tyt20")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, "camera_select.npz")) as z:
        return {k: z[k] for k in z.files}


def views_of(name):
    return {i: {"world_mat": m} for i, m in enumerate(golden()[f"{name}_world_mat"])}


def cloud(n, seed):
    """n centred points in three unequal blobs, no two alike."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3)) * np.array([1.5, 1.0, 0.5]) + 2.0 * rng.integers(-1, 2, size=(n, 1)) * np.array([1.0, -0.5, 0.25])
    return x - x.mean(axis=0)


def inits(X, ks, seed=42):
    """k-means++ centres for every k of ks from one RandomState: [len(ks),GSR_CK_KMAX,3]."""
    rs = np.random.RandomState(seed)
    out = np.zeros((len(ks), GSR_CK_KMAX, 3))
    for f, k in enumerate(ks):
        out[f, :k] = CS.kmeans_pp_init(X, k, rs)
    return out


def tolerance(X):
    return float(np.mean(np.var(X, axis=0)) * CS.TOL)


# ---------------------------------------------------------------- the scan of the command tests
def scan8(root, n_points=300):
    """A dtu scan of the golden set dome8: eight 96x128 pictures, cameras.npz with those world_mats, and 300 points around the
    origin that every camera sees inside its picture (camera_mat maps +-0.6 to the frame).  -> the points."""
    from PIL import Image
    from gaussmart_amd import segment_cli
    rng = np.random.default_rng(11)
    os.makedirs(os.path.join(root, "images"))
    yy, xx = np.mgrid[0:96, 0:128]
    mats = {}
    for i, world in enumerate(golden()["dome8_world_mat"]):
        img = np.stack([(xx * 2 + 23 * i) % 256, (yy * 2 + 11 * i) % 256, ((xx // 16 + yy // 16 + i) % 2) * 200], -1).astype(np.uint8)
        img[20 + 3 * i:60, 30 + 5 * i:90] = (250, 30 + 20 * i, 30)
        Image.fromarray(img).save(os.path.join(root, "images", f"{i:04d}.png"))
        mats[f"world_mat_{i}"], mats[f"scale_mat_{i}"] = world, np.eye(4)
        mats[f"camera_mat_{i}"] = np.array([[80.0, 0, 64, 0], [0, 60.0, 48, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    np.savez(os.path.join(root, "cameras.npz"), **mats)
    pts = rng.uniform(-0.4, 0.4, (n_points, 3))
    segment_cli.write_cloud_ply(os.path.join(root, "points.ply"), pts, np.full((n_points, 3), 200, np.uint8))
    return pts


class StubGenerator:
    """generate_segments of the SAM generators without a model: three rectangles that move with the picture's content."""
    last_ms = {}

    def generate_segments(self, image):
        h, w = image.shape[:2]
        s = int(image[..., 1].sum()) % 7
        masks = np.zeros((3, h, w), bool)
        boxes = np.array([[5 + s, 4, 70, 50 + s], [60, 30 + s, 120, 90], [20, 60, 50 + s, 80]], np.int64)
        for m, (x0, y0, x1, y1) in zip(masks, boxes):
            m[y0:y1 + 1, x0:x1 + 1] = True
        return masks.view(np.uint8), dict(masks=masks, boxes=boxes, areas=masks.sum(axis=(1, 2)).astype(np.int64))
