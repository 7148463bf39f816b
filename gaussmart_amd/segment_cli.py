"""Label a scan's point cloud by view masks: steps 3-5 of the reference's identification/main.py (hull filter, projection
into the selected views, segment labels and mask areas) on the device, from masks that already exist.

    python -m gaussmart_amd.segment_cli -s SCAN -o OUT -t dtu|nerf|tyt --masks DIR --views i j k ... [--clean] [--host]

Reads the point cloud (`points.ply` for dtu, `sparse/0/points3D.ply` otherwise), the cameras (`cameras.npz` for dtu,
`poses_bounds.npy` otherwise, in the layouts of identification/camera_loader.py) and the masks `DIR/segments_NNN.npz` (key
`masks`, [M,H,W]; the k-th file belongs to the k-th --views entry).  Writes, under OUT/segments/point_cloud/, what the
reference writes there: raw_pc.ply, segmented_point_cloud.ply, segment_indices.npy and mask_areas.npy (a pickled dict).
`--segmentation_dir OUT/segments/point_cloud` of gaussmart_amd.train_cli reads them.  --host runs the numpy twins.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import segment_init as SI
from .camera_select import NERF_IMG_WH, TYT_FOCAL, TYT_IMG_WH, load_cameras  # noqa: F401  (load_cameras lives there now)
from .scene_io import read_ply_vertices


def write_cloud_ply(path, points, colors=None, normals=None):
    """x y z (double), nx ny nz (double) and red green blue (uchar) where present: the columns Open3D writes."""
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if normals is not None:
        fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    el = np.zeros(len(points), dtype=np.dtype(fields))
    el["x"], el["y"], el["z"] = np.asarray(points, np.float64).reshape(-1, 3).T
    if normals is not None:
        el["nx"], el["ny"], el["nz"] = np.asarray(normals, np.float64).reshape(-1, 3).T
    if colors is not None:
        el["red"], el["green"], el["blue"] = np.asarray(colors, np.uint8).reshape(-1, 3).T
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(el)
    header += "".join(f"property {'uchar' if t == 'u1' else 'double'} {k}\n" for k, t in fields) + "end_header\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(el.tobytes())


def read_cloud(path):
    """(points [n,3] in the file's own precision, colors uint8 [n,3] or None, normals [n,3] or None)."""
    v = read_ply_vertices(path)
    names = v.dtype.names
    pts = np.stack([v["x"], v["y"], v["z"]], axis=1)
    col = np.stack([v["red"], v["green"], v["blue"]], axis=1) if "red" in names else None
    nrm = np.stack([v["nx"], v["ny"], v["nz"]], axis=1) if "nx" in names else None
    return np.ascontiguousarray(pts), col, nrm


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-s", "--scan_path", required=True)
    ap.add_argument("-o", "--output_path", required=True)
    ap.add_argument("-t", "--type", choices=sorted(SI.KINDS), required=True)
    ap.add_argument("--masks", required=True, help="directory with segments_NNN.npz (key `masks`), one per --views entry")
    ap.add_argument("--views", type=int, nargs="+", required=True, help="camera indices of the mask files, in their order")
    ap.add_argument("--clean", action="store_true", help="apply the convex-hull filter first")
    ap.add_argument("--theta", type=float, default=SI.THETA)
    ap.add_argument("--host", action="store_true", help="numpy twins instead of the HIP kernels")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dump_projection", type=int, default=None, metavar="K",
                    help="also write projection_KKK.npz (uv, z) of the K-th --views entry")
    args = ap.parse_args(argv)

    kind = args.type
    pc_path = os.path.join(args.scan_path, "points.ply" if kind == "dtu" else os.path.join("sparse", "0", "points3D.ply"))
    cam_path = os.path.join(args.scan_path, "cameras.npz" if kind == "dtu" else "poses_bounds.npy")
    points, colors, normals = read_cloud(pc_path)
    all_cameras = load_cameras(cam_path, kind)
    missing = [i for i in args.views if i not in all_cameras]
    if missing:
        raise SystemExit(f"--views {missing} are not in {cam_path} ({len(all_cameras)} cameras)")
    cameras = [all_cameras[i] for i in args.views]
    masks = []
    for k in range(len(args.views)):
        with np.load(os.path.join(args.masks, f"segments_{k:03d}.npz")) as z:
            masks.append(np.asarray(z["masks"]))

    out_dir = os.path.join(args.output_path, "segments", "point_cloud")
    os.makedirs(out_dir, exist_ok=True)
    n_in = len(points)
    if args.host:
        if args.clean:
            _, points, colors, normals = SI.hull_filter_host(points, args.theta, colors, normals)
        labels, areas = SI.label_points_host(points, cameras, kind, masks)
    else:
        import torch
        dev = torch.device(args.device)
        if args.clean:
            keep, _, _, _ = SI.hull_filter(points, args.theta, device=dev)
            keep = keep.cpu().numpy()
            points, colors, normals = points[keep], None if colors is None else colors[keep], None if normals is None else normals[keep]
        labels, areas = SI.label_points(points, cameras, kind, masks, device=dev)
        labels = labels.cpu().numpy()
    if args.dump_projection is not None:
        cam = cameras[args.dump_projection]
        if args.host:
            uv, z = SI.project_points_host(points, cam, kind)
        else:
            uv, z = (t.cpu().numpy() for t in SI.project_points(points, cam, kind, device=dev))
        np.savez(os.path.join(out_dir, f"projection_{args.dump_projection:03d}.npz"), uv=uv, z=z)
    write_cloud_ply(os.path.join(out_dir, "raw_pc.ply"), points, colors, normals)
    write_cloud_ply(os.path.join(out_dir, "segmented_point_cloud.ply"), points, colors, normals)
    np.save(os.path.join(out_dir, "segment_indices.npy"), labels.astype(np.int64))
    np.save(os.path.join(out_dir, "mask_areas.npy"), areas)
    print(json.dumps({"points_in": n_in, "points": len(points), "labelled": int((labels >= 0).sum()), "segments": len(areas),
                      "views": len(cameras), "host": bool(args.host)}))


if __name__ == "__main__":
    sys.exit(main())
