"""Score a mesh (or a point cloud) against a DTU scan: the reference's scripts/eval_dtu/eval.py, with its arguments.

    python -m gaussmart_amd.dtu_eval_cli --data M.ply --scan 24 --dataset_dir DTU --vis_out_dir OUT [--mode mesh|pcd]
                                         [--downsample_density 0.2] [--patch_size 60] [--max_dist 20]
                                         [--visualize_threshold 10] [--seed 0] [--host] [--write_vis]

Writes OUT/results.json (mean_d2s, mean_s2d, overall) and prints the three numbers; with --write_vis also the two coloured
clouds OUT/vis_{scan:03}_d2s.ply and OUT/vis_{scan:03}_s2d.ply.  --seed picks the shuffle that precedes the down-sampling."""
import argparse
import json
import os
import sys

import numpy as np

from . import _lib
from . import mesh_eval as ME
from .mesh import TriangleMesh


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Chamfer distance of a mesh to a DTU scan.")
    ap.add_argument("--data", type=str, default="data_in.ply", help="binary PLY: the mesh (or the cloud with --mode pcd)")
    ap.add_argument("--scan", type=int, default=1)
    ap.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    ap.add_argument("--dataset_dir", type=str, default=".")
    ap.add_argument("--vis_out_dir", type=str, default=".")
    ap.add_argument("--downsample_density", type=float, default=ME.DEFAULT_DENSITY)
    ap.add_argument("--patch_size", type=float, default=ME.DEFAULT_PATCH)
    ap.add_argument("--max_dist", type=float, default=ME.DEFAULT_MAX_DIST)
    ap.add_argument("--visualize_threshold", type=float, default=ME.DEFAULT_VIS_DIST)
    ap.add_argument("--seed", type=int, default=0, help="seed of the shuffle before the down-sampling")
    ap.add_argument("--host", action="store_true", help="numpy + scipy instead of the device kernels")
    ap.add_argument("--write_vis", action="store_true", help="also write the two error-coloured clouds")
    args = ap.parse_args(argv)
    try:
        if not os.path.isfile(args.data):
            raise FileNotFoundError(f"{args.data}: no such file")
        inst = ME.load_dtu_eval_instance(args.dataset_dir, args.scan)
        mesh = TriangleMesh.read_ply(args.data)
        kw = dict(downsample_density=args.downsample_density, patch_size=args.patch_size, max_dist=args.max_dist)
        if args.mode == "mesh":
            data = mesh
            cloud = ME.sample_mesh_points_host(mesh, args.downsample_density) if args.host else None
        else:
            data = cloud = mesh.vertices
        if args.host:
            order = ME.default_order(len(cloud), args.seed)
            res = ME.evaluate_dtu_mesh_host(cloud, order=order, **inst, **kw)
        else:
            import torch
            if not torch.cuda.is_available():
                raise _lib.GsrError("no GPU: the device path has no CPU fall-back (use --host)")
            dev = torch.device("cuda", 0)
            if cloud is None:
                cloud = ME.sample_mesh_points(data, args.downsample_density, device=dev)
            order = ME.default_order(len(cloud), args.seed)
            res = ME.evaluate_dtu_mesh(cloud, order=order, device=dev, **inst, **kw)
        out = {k: float(res[k]) for k in ("mean_d2s", "mean_s2d", "overall")}
        os.makedirs(args.vis_out_dir, exist_ok=True)
        with open(os.path.join(args.vis_out_dir, "results.json"), "w") as f:
            json.dump(out, f, indent=True)
        if args.write_vis:
            down, stl = _host(res["data_down"]), inst["stl_points"]
            rows = np.nonzero(_host(res["in_obs"]))[0]
            col = ME.error_colors(len(down), rows, _host(res["dist_d2s"]), args.max_dist, args.visualize_threshold)
            TriangleMesh(down, None, col).write_ply(os.path.join(args.vis_out_dir, f"vis_{args.scan:03}_d2s.ply"))
            rows = np.nonzero(_host(res["above"]))[0]
            col = ME.error_colors(len(stl), rows, _host(res["dist_s2d"]), args.max_dist, args.visualize_threshold)
            TriangleMesh(stl, None, col).write_ply(os.path.join(args.vis_out_dir, f"vis_{args.scan:03}_s2d.ply"))
    except (OSError, ValueError, KeyError, _lib.GsrError) as e:
        print(f"dtu_eval_cli: {e}", file=sys.stderr)
        return 2
    print(out["mean_d2s"], out["mean_s2d"], out["overall"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
