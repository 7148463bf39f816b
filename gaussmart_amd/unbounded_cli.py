"""Command-line mesh export for unbounded scenes, the counterpart of the reference's `render.py --unbounded`:

    python -m gaussmart_amd.unbounded_cli -s <scene> -m <model dir> [--iteration -1] [--depth_ratio R] [--mesh_res 1024]
        [--mesh_crop 512] [--num_cluster 50] [--host_post_process] [--host]

Always meshes unbounded (mesh_unbounded.UnboundedExtractor) and writes MODEL/train/ours_<it>/fuse_unbounded.ply and
fuse_unbounded_post.ply, the reference's names.  The mesh stays on the device from the field to the PLY writer;
--host_post_process runs the numpy + scipy cluster filter instead.  --host loads the model on the CPU and runs the torch
twins of the field, the lattice and marching cubes (small --mesh_res only: the lattice is held densely, and the renderer
still needs the device for the depth maps).  Images are exported by render_cli.
"""
import argparse
import os

import torch

from .gaussian_model import GaussianModel
from .gaussian_renderer import render
from .mesh import post_process_mesh, post_process_mesh_device
from .mesh_unbounded import UnboundedExtractor, marching_cubes_contracted_host, quantile_radius
from .params import PipelineParams
from .scene_io import Scene


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source_path", "-s", required=True)
    ap.add_argument("--model_path", "-m", required=True)
    ap.add_argument("--images", "-i", default=None)
    ap.add_argument("--resolution", "-r", type=int, default=-1)
    ap.add_argument("--white_background", "-w", action="store_true")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--sh_degree", type=int, default=3)
    ap.add_argument("--depth_ratio", type=float, default=0.0)
    ap.add_argument("--iteration", default=-1, type=int)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--num_cluster", default=50, type=int, help="Mesh: number of connected clusters to export")
    ap.add_argument("--unbounded", action="store_true", help="accepted for render.py's command lines; always on here")
    ap.add_argument("--mesh_res", default=1024, type=int, help="Mesh: resolution for unbounded mesh extraction")
    ap.add_argument("--mesh_crop", default=512, type=int, help="Mesh: points per crop of the lattice (the reference: 512)")
    ap.add_argument("--host_post_process", action="store_true",
                    help="Mesh: filter the clusters on the host (numpy + scipy) instead of on the device")
    ap.add_argument("--host", action="store_true", help="Mesh: run the torch CPU twins of the field and of marching cubes")
    args = ap.parse_args(argv)
    print("Rendering " + args.model_path)

    dev = torch.device("cuda", torch.cuda.current_device())
    pipe = PipelineParams(depth_ratio=args.depth_ratio)
    gaussians = GaussianModel(args.sh_degree, device=dev)
    scene = Scene(args.source_path, gaussians, model_path=args.model_path, load_iteration=args.iteration,
                  images=args.images, eval=args.eval, white_background=args.white_background, resolution=args.resolution,
                  data_device=dev, shuffle=False)
    bg_color = [1, 1, 1] if args.white_background else [0, 0, 0]
    train_dir = os.path.join(args.model_path, "train", f"ours_{scene.loaded_iter}")
    ex = UnboundedExtractor(gaussians, render, pipe, bg_color=bg_color)

    print("export mesh ...")
    os.makedirs(train_dir, exist_ok=True)
    ex.gaussians.active_sh_degree = 0   # diffuse texture only
    ex.reconstruction(scene.getTrainCameras())
    name = "fuse_unbounded.ply"
    if args.host:
        R = quantile_radius(gaussians.get_xyz.cpu(), ex.center, ex.radius)
        views = [(M, d.cpu(), c.cpu()) for M, d, c in ex.views()]
        mesh = marching_cubes_contracted_host(views, ex.center, ex.radius, R, args.mesh_res, args.mesh_crop)
    else:
        mesh = ex.extract_mesh_unbounded(resolution=args.mesh_res, crop=args.mesh_crop, to_host=False)
        if args.host_post_process:
            mesh = mesh.cpu()
    mesh.write_ply(os.path.join(train_dir, name))
    print("mesh saved at {}".format(os.path.join(train_dir, name)))
    post = post_process_mesh if (args.host or args.host_post_process) else post_process_mesh_device
    mesh_post = post(mesh, cluster_to_keep=args.num_cluster)
    mesh_post.write_ply(os.path.join(train_dir, name.replace(".ply", "_post.ply")))
    print("mesh post processed saved at {}".format(os.path.join(train_dir, name.replace(".ply", "_post.ply"))))


if __name__ == "__main__":
    main()
