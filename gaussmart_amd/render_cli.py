"""Command-line rendering, mesh export and trajectory videos, the counterpart of the reference's render.py (bounded TSDF path):

    python -m gaussmart_amd.render_cli -s <scene> -m <model dir> [--iteration -1] [--skip_train] [--skip_test]
        [--skip_mesh] [--voxel_size V] [--depth_trunc D] [--sdf_trunc S] [--num_cluster 50] [--mesh_res 1024]
        [--depth_ratio R] [--host_post_process] [--render_path [--n_frames 240] [--host]]

Writes MODEL/{train,test}/ours_<it>/{renders,gt,vis} and MODEL/train/ours_<it>/fuse.ply, fuse_post.ply (what the reference's
scripts/dtu_eval_mesh.py reads).  The mesh stays on the device from marching cubes to the PLY writer (cluster filter as
kernels); --host_post_process runs the numpy + scipy filter instead and writes the same bytes.

--render_path (render.py:73-84) renders --n_frames views on an ellipse through the training cameras
(gaussmart_amd/render_path.py) and writes MODEL/traj/ours_<it>/{renders,vis}, render_traj_color.avi and render_traj_depth.avi
(Motion-JPEG; the reference's .mp4 where mediapy is installed).  The frames are converted by kernels next to the maps
(gaussmart_amd/frames.py); --host converts with numpy and makes the videos from the files, like the reference.

--unbounded is not supported here; `python -m gaussmart_amd.unbounded_cli` meshes unbounded scenes.
"""
import argparse
import os
import sys

import torch

from .gaussian_model import GaussianModel
from .gaussian_renderer import render
from .mesh import GaussianExtractor, post_process_mesh, post_process_mesh_device
from .params import PipelineParams
from .render_path import generate_path
from .scene_io import Scene
from .video import export_trajectory


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
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_test", action="store_true")
    ap.add_argument("--skip_mesh", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--render_path", action="store_true", help="render a fly-around of the scene and make videos of it")
    ap.add_argument("--n_frames", default=240, type=int, help="Trajectory: number of frames")
    ap.add_argument("--host", action="store_true",
                    help="Trajectory: convert the frames on the host and make the videos from the written files")
    ap.add_argument("--voxel_size", default=-1.0, type=float, help="Mesh: voxel size for TSDF")
    ap.add_argument("--depth_trunc", default=-1.0, type=float, help="Mesh: Max depth range for TSDF")
    ap.add_argument("--sdf_trunc", default=-1.0, type=float, help="Mesh: truncation value for TSDF")
    ap.add_argument("--num_cluster", default=50, type=int, help="Mesh: number of connected clusters to export")
    ap.add_argument("--unbounded", action="store_true", help="Mesh: using unbounded mode for meshing (not supported)")
    ap.add_argument("--host_post_process", action="store_true",
                    help="Mesh: filter the clusters on the host (numpy + scipy) instead of on the device")
    ap.add_argument("--mesh_res", default=1024, type=int, help="Mesh: resolution for unbounded mesh extraction")
    args = ap.parse_args(argv)
    if args.unbounded:
        sys.exit("render_cli: --unbounded is not supported (only the bounded TSDF mesh path is implemented here); "
                 "`python -m gaussmart_amd.unbounded_cli` with the same arguments meshes an unbounded scene")
    print("Rendering " + args.model_path)

    dev = torch.device("cuda", torch.cuda.current_device())
    pipe = PipelineParams(depth_ratio=args.depth_ratio)
    gaussians = GaussianModel(args.sh_degree, device=dev)
    scene = Scene(args.source_path, gaussians, model_path=args.model_path, load_iteration=args.iteration,
                  images=args.images, eval=args.eval, white_background=args.white_background, resolution=args.resolution,
                  data_device=dev, shuffle=False)
    bg_color = [1, 1, 1] if args.white_background else [0, 0, 0]
    train_dir = os.path.join(args.model_path, "train", f"ours_{scene.loaded_iter}")
    test_dir = os.path.join(args.model_path, "test", f"ours_{scene.loaded_iter}")
    ex = GaussianExtractor(gaussians, render, pipe, bg_color=bg_color)

    if not args.skip_train:
        print("export training images ...")
        os.makedirs(train_dir, exist_ok=True)
        ex.reconstruction(scene.getTrainCameras())
        ex.export_image(train_dir)
    if not args.skip_test and len(scene.getTestCameras()) > 0:
        print("export rendered testing images ...")
        os.makedirs(test_dir, exist_ok=True)
        ex.reconstruction(scene.getTestCameras())
        ex.export_image(test_dir)

    if args.render_path:
        print("render videos ...")
        traj_dir = os.path.join(args.model_path, "traj", f"ours_{scene.loaded_iter}")
        os.makedirs(traj_dir, exist_ok=True)
        ex.reconstruction(generate_path(scene.getTrainCameras(), n_frames=args.n_frames))
        export_trajectory(ex, traj_dir, "render_traj", host=args.host)

    if not args.skip_mesh:
        print("export mesh ...")
        os.makedirs(train_dir, exist_ok=True)
        ex.gaussians.active_sh_degree = 0   # diffuse texture only
        ex.reconstruction(scene.getTrainCameras())
        name = "fuse.ply"
        depth_trunc = (ex.radius * 2.0) if args.depth_trunc < 0 else args.depth_trunc
        voxel_size = (depth_trunc / args.mesh_res) if args.voxel_size < 0 else args.voxel_size
        sdf_trunc = 5.0 * voxel_size if args.sdf_trunc < 0 else args.sdf_trunc
        mesh = ex.extract_mesh_bounded(voxel_size=voxel_size, sdf_trunc=sdf_trunc, depth_trunc=depth_trunc, aabb="device",
                                       to_host=False)
        if args.host_post_process:
            mesh = mesh.cpu()
        mesh.write_ply(os.path.join(train_dir, name))
        print("mesh saved at {}".format(os.path.join(train_dir, name)))
        post = post_process_mesh if args.host_post_process else post_process_mesh_device
        mesh_post = post(mesh, cluster_to_keep=args.num_cluster)
        mesh_post.write_ply(os.path.join(train_dir, name.replace(".ply", "_post.ply")))
        print("mesh post processed saved at {}".format(os.path.join(train_dir, name.replace(".ply", "_post.ply"))))


if __name__ == "__main__":
    main()
