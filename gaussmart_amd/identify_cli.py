"""The reference's identification/main.py, steps 1 to 5, in one process:

    python -m gaussmart_amd.identify_cli -s SCAN -o OUT -t dtu|nerf|tyt [--skip_camera_clustering] [--sam2] [--clean]
        --sam_checkpoint FILE_OR_DIR [--decoder torch|hip] [--model_type ...] [--points_per_side 32] [--pred_iou_thresh 0.86]
        [--stability_score_thresh 0.92] [--theta 1.96] [--host] [--device cuda] [--overwrite]

  1. the views: k-means over the camera centres for k = 3 .. 15, one representative camera per cluster of the best-scoring k
     (gaussmart_amd.camera_select; all fits in one launch of gsr_cam_lloyd), or every view with --skip_camera_clustering;
  2. SAM / SAM2 masks of those views (gaussmart_amd.sam / sam2, as gaussmart_amd.sam_cli);
  3. the point cloud, through the convex-hull filter with --clean;
  4. projection into the views and the segment labels (gaussmart_amd.segment_init, as gaussmart_amd.segment_cli);
  5. the files.
It writes the reference's tree: OUT/segments/{images,masks,point_cloud,embeddings,cameras} with cameras/selected_cameras.npz
(selected_indices and cameras_dict as np.savez stores them: the second is a pickled dict), masks/segments_NNN.npz (masks, boxes,
areas), point_cloud/{raw_pc.ply, segmented_point_cloud.ply, segment_indices.npy, mask_areas.npy} and the selected pictures under
their own names.  Each view's masks go from the generator to the labelling as device tensors; the .npz is written from one copy
to the host.  One JSON line per step with its time, and a last one with the selected views.

Where this command differs from the reference: the reference deletes an existing OUT/segments; this command refuses it unless
--overwrite is given.  Fewer than 4 cameras (the reference fails inside scikit-learn) and a missing picture (the reference warns
and goes on with the views out of step) are errors.  --host runs the numpy twins of steps 1, 3 and 4 and the torch modules of
step 2.
"""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

from . import camera_select as CS
from . import segment_init as SI
from .segment_cli import read_cloud, write_cloud_ply

DIRS = ("images", "masks", "point_cloud", "embeddings", "cameras")


def scan_paths(scan_path, kind):
    """(point cloud, cameras, image directory) of a scan (identification/main.py:44-57)."""
    if kind == "dtu":
        return os.path.join(scan_path, "points.ply"), os.path.join(scan_path, "cameras.npz"), os.path.join(scan_path, "images")
    return os.path.join(scan_path, "sparse", "0", "points3D.ply"), os.path.join(scan_path, "poses_bounds.npy"), os.path.join(scan_path, "images")


def add_arguments(ap):
    """The flags this command shares with gaussmart_amd.train_cli --run_segmentation."""
    ap.add_argument("--skip_camera_clustering", action="store_true", help="select every view")
    ap.add_argument("--sam2", action="store_true", help="SAM2 (Hiera) instead of SAM; --sam_checkpoint is then a local directory")
    ap.add_argument("--clean", action="store_true", help="apply the convex-hull filter to the point cloud first")
    ap.add_argument("--sam_checkpoint", default=None, help="a local .pth (segment_anything) or directory (transformers); never downloaded")


def run(args, generator=None, echo=print):
    """The pipeline for parsed arguments.  generator: an object with generate_segments(image) and last_ms instead of the SAM /
    SAM2 generator the arguments name.  -> dict(selected, labels, mask_areas, point_cloud_dir)."""
    kind = args.type
    pc_path, cam_path, image_dir = scan_paths(args.scan_path, kind)
    base = os.path.join(args.output_path, "segments")
    if os.path.exists(base) and not args.overwrite:
        raise SystemExit(f"identify_cli: {base} exists; the reference would delete it, this command only does so with --overwrite")
    for path, what in ((cam_path, "cameras"), (image_dir, "images"), (pc_path, "point cloud")):
        if not os.path.exists(path):
            raise SystemExit(f"identify_cli: {path} ({what}) does not exist")
    device = None if args.host else args.device

    def step(number, name, t0, **info):
        echo(json.dumps({"step": number, "name": name, "ms": round(1e3 * (time.perf_counter() - t0), 3), **info}))

    # 1. the views
    t0 = time.perf_counter()
    details = {}
    try:
        selected, views = CS.select_views(cam_path, kind, cluster=not args.skip_camera_clustering, device=device, details=details)
    except ValueError as e:
        raise SystemExit(f"identify_cli: {e}")
    missing = [i for i in selected if i not in views]
    if missing:
        raise SystemExit(f"identify_cli: selected views {missing} are not among the {len(views)} cameras of {cam_path}")
    files = CS.list_images(image_dir)
    try:
        images = [CS.image_path(image_dir, kind, i, files) for i in selected]
    except FileNotFoundError as e:
        raise SystemExit(f"identify_cli: {e}")
    cameras = [views[i] for i in selected]
    if os.path.exists(base):
        shutil.rmtree(base)
    dirs = {d: os.path.join(base, d) for d in DIRS}
    for d in dirs.values():
        os.makedirs(d)
    np.savez(os.path.join(dirs["cameras"], "selected_cameras.npz"), selected_indices=selected,
             cameras_dict={f"camera_{k:03d}": cam for k, cam in enumerate(cameras)})
    step(1, "select_views", t0, cameras=len(views), selected=len(selected), best_k=details.get("best_k"), host=bool(args.host),
         clustered=not args.skip_camera_clustering)

    # 2. the masks
    t0 = time.perf_counter()
    if generator is None:
        if not args.sam_checkpoint:
            raise SystemExit("identify_cli: --sam_checkpoint is required (a local file or directory; nothing is downloaded)")
        from .sam_cli import make_generator
        generator = make_generator(args)[0]
    from PIL import Image
    masks_per_view, per_view = [], []
    for k, path in enumerate(images):
        image = np.asarray(Image.open(path).convert("RGB"))
        masks, host = generator.generate_segments(image)
        np.savez(os.path.join(dirs["masks"], f"segments_{k:03d}.npz"), masks=host["masks"], boxes=host["boxes"], areas=host["areas"])
        shutil.copy2(path, os.path.join(dirs["images"], os.path.basename(path)))
        masks_per_view.append(host["masks"] if args.host else masks)
        per_view.append({"view": selected[k], "image": os.path.basename(path), "masks": int(len(host["areas"])),
                         **{f"{n}_ms": round(ms, 3) for n, ms in getattr(generator, "last_ms", {}).items()}})
    step(2, "masks", t0, views=per_view)

    # 3. the point cloud
    t0 = time.perf_counter()
    points, colors, normals = read_cloud(pc_path)
    n_in = len(points)
    if args.clean:
        if args.host:
            _, points, colors, normals = SI.hull_filter_host(points, args.theta, colors, normals)
        else:
            keep = SI.hull_filter(points, args.theta, device=device)[0].cpu().numpy()
            points, colors, normals = points[keep], None if colors is None else colors[keep], None if normals is None else normals[keep]
    write_cloud_ply(os.path.join(dirs["point_cloud"], "raw_pc.ply"), points, colors, normals)
    step(3, "point_cloud", t0, points_in=n_in, points=len(points), clean=bool(args.clean))

    # 4. projection and labels
    t0 = time.perf_counter()
    if args.host:
        labels, areas = SI.label_points_host(points, cameras, kind, masks_per_view)
    else:
        labels, areas = SI.label_points(points, cameras, kind, masks_per_view, device=device)
        labels = labels.cpu().numpy()
    step(4, "labels", t0, labelled=int((labels >= 0).sum()), segments=len(areas))

    # 5. the files
    t0 = time.perf_counter()
    write_cloud_ply(os.path.join(dirs["point_cloud"], "segmented_point_cloud.ply"), points, colors, normals)
    np.save(os.path.join(dirs["point_cloud"], "segment_indices.npy"), labels.astype(np.int64))
    np.save(os.path.join(dirs["point_cloud"], "mask_areas.npy"), areas)
    step(5, "files", t0, out=base)
    echo(json.dumps({"selected_views": selected, "images": [os.path.basename(p) for p in images], "points": len(points),
                     "labelled": int((labels >= 0).sum()), "segments": len(areas), "host": bool(args.host)}))
    return dict(selected=selected, labels=labels, mask_areas=areas, point_cloud_dir=dirs["point_cloud"])


def parser():
    ap = argparse.ArgumentParser(prog="gaussmart_amd.identify_cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-s", "--scan_path", required=True)
    ap.add_argument("-o", "--output_path", required=True)
    ap.add_argument("-t", "--type", choices=sorted(SI.KINDS), required=True)
    add_arguments(ap)
    ap.add_argument("--model_type", choices=("vit_h", "vit_l", "vit_b", "large", "base_plus", "small", "tiny"), default=None,
                    help="checked against the checkpoint's own shape when given (vit_*: SAM; the others: --sam2)")
    ap.add_argument("--decoder", choices=("torch", "hip"), default="torch", help="the prompt encoder and mask decoder: transformers' or the kernels")
    ap.add_argument("--points_per_side", type=int, default=32)
    ap.add_argument("--pred_iou_thresh", type=float, default=0.86)
    ap.add_argument("--stability_score_thresh", type=float, default=0.92)
    ap.add_argument("--theta", type=float, default=SI.THETA, help="the hull filter's threshold in standard deviations (--clean)")
    ap.add_argument("--host", action="store_true", help="numpy twins of steps 1, 3 and 4, the torch modules of step 2")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--overwrite", action="store_true", help="delete an existing OUT/segments first (the reference always does)")
    return ap


def main(argv=None, generator=None):
    run(parser().parse_args(argv), generator)
    return 0


if __name__ == "__main__":
    sys.exit(main())
