"""Command-line training entry: the build's counterpart of the reference's train.py / render.py
front ends for the hot path (scene in -> optimised surfels + PSNR out).  SAM preprocessing,
TensorBoard and the viewer socket of the reference are out of scope; SSIM, PSNR
and LPIPS of the rendered test views come from gaussmart_amd.metrics_cli, not from this command.
The reference's DINO feature term is behind --dino_dir (a LOCAL directory with the DINOv3 ViT weights; nothing
is downloaded): it is logged to MODEL/dino_loss_log.csv and carries no gradient, as in the reference.

    python -m gaussmart_amd.train_cli -s <colmap-or-blender-scene> -m <output dir> [--iterations 30000] [--eval]
        [--dino_dir DIR [--lambda_dino 0.05] [--dino_start_iter 3000] [--host]]
        [--run_segmentation --dataset_type dtu|nerf|tyt --sam_checkpoint FILE_OR_DIR [--skip_camera_clustering] [--sam2] [--clean]]
    torchrun --nproc-per-node 8 -m gaussmart_amd.train_cli -s ... -m ...        # view-parallel

--run_segmentation is the reference's train.py:362-367,380-406: before training, steps 1 to 5 of identification/main.py run in this
process (gaussmart_amd.identify_cli: view selection, SAM / SAM2 masks, labels) into MODEL/segmentation, and --segmentation_dir is set
to the result unless one was given.
"""
import argparse
import json
import os
import time

import torch

from . import identify_cli
from .gaussian_model import GaussianModel
from .gaussian_renderer import render
from .losses import psnr
from .params import OptimizationParams, PipelineParams
from .scene_io import Scene
from .trainer import train, TrainState, DinoTerm
from .view_parallel import ViewParallel


def evaluate(gaussians, cameras, pipe, background):
    vals = []
    with torch.no_grad():
        for cam in cameras:
            img = render(cam, gaussians, pipe, background, surface_maps=False)["render"].clamp(0, 1)
            vals.append(psnr(img[None], cam.original_image.to(img.device)[None]).mean())
    return float(torch.stack(vals).mean()) if vals else float("nan")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source_path", "-s", required=True)
    ap.add_argument("--model_path", "-m", required=True)
    ap.add_argument("--images", "-i", default=None)
    ap.add_argument("--resolution", "-r", type=int, default=-1)
    ap.add_argument("--white_background", "-w", action="store_true")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--sh_degree", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=30_000)
    ap.add_argument("--save_iterations", type=int, nargs="*", default=[7000, 30000])
    ap.add_argument("--depth_ratio", type=float, default=0.0)
    ap.add_argument("--lambda_normal", type=float, default=0.05)
    ap.add_argument("--lambda_dist", type=float, default=0.0)
    ap.add_argument("--start_checkpoint", default=None)
    ap.add_argument("--log_every", type=int, default=500)
    ap.add_argument("--segmentation_dir", default=None,
                    help="directory with segment_indices.npy / mask_areas.npy (gaussmart_amd.segment_cli's OUT/segments/point_cloud): "
                         "the initial cloud is augmented per segment")
    ap.add_argument("--run_segmentation", action="store_true",
                    help="run gaussmart_amd.identify_cli on the scene first (into MODEL/segmentation) and train from its labels")
    ap.add_argument("--dataset_type", choices=("dtu", "nerf", "tyt"), default="tyt", help="with --run_segmentation: the scan's layout")
    identify_cli.add_arguments(ap)
    ap.add_argument("--uniform_upsampling", action="store_true",
                    help="without mask areas: augment the initial cloud as one segment")
    ap.add_argument("--dino_dir", default=None,
                    help="local directory with config.json, preprocessor_config.json and model.safetensors of a DINOv3 ViT: adds "
                         "the reference's DINO feature term to the logged total loss (MODEL/dino_loss_log.csv); never a hub name")
    ap.add_argument("--lambda_dino", type=float, default=0.05)
    ap.add_argument("--dino_start_iter", type=int, default=3000)
    ap.add_argument("--host", action="store_true",
                    help="with --dino_dir: run the encoder through transformers' model (torch) instead of the HIP kernels")
    args = ap.parse_args(argv)

    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    torch.manual_seed(0)

    if args.run_segmentation:
        seg_out = os.path.join(args.model_path, "segmentation")
        if rank == 0:
            seg_args = ["-s", args.source_path, "-o", seg_out, "-t", args.dataset_type, "--device", str(dev), "--overwrite"]
            seg_args += [f"--{name}" for name in ("skip_camera_clustering", "sam2", "clean") if getattr(args, name)]
            seg_args += ["--sam_checkpoint", args.sam_checkpoint] if args.sam_checkpoint else []
            identify_cli.main(seg_args)
        if world > 1:
            dist.barrier()
        if args.segmentation_dir is None:
            args.segmentation_dir = os.path.join(seg_out, "segments", "point_cloud")

    opt = OptimizationParams(iterations=args.iterations, lambda_normal=args.lambda_normal, lambda_dist=args.lambda_dist)
    pipe = PipelineParams(depth_ratio=args.depth_ratio)
    gaussians = GaussianModel(args.sh_degree, uniform_upsampling=args.uniform_upsampling, device=dev)
    scene = Scene(args.source_path, gaussians, model_path=args.model_path, images=args.images, eval=args.eval,
                  white_background=args.white_background, resolution=args.resolution, data_device=dev,
                  segmentation_dir=args.segmentation_dir)
    gaussians.training_setup(opt)
    first_iter = 0
    if args.start_checkpoint:
        # capture() holds ints, floats, tensors / Parameters and the optimiser's state_dict: the weights-only loader
        # (no arbitrary pickle code from the file) is sufficient
        model_params, first_iter = torch.load(args.start_checkpoint, map_location=dev, weights_only=True)
        gaussians.restore(model_params, opt)
    background = torch.tensor([1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0], device=dev)
    # one rank: no exchange; past the densification phase train() takes the same pipelined step as N > 1 (SH update on a
    # side stream beside the next forward's binning), before it the serial step behind the densification bookkeeping
    vp = ViewParallel(gaussians) if world > 1 else ViewParallel(gaussians, overlap_local=True)

    os.makedirs(args.model_path, exist_ok=True)
    dino = None
    if args.dino_dir and rank == 0:
        from .dino import DINOImageEncoder, HostDINOImageEncoder
        encoder = (HostDINOImageEncoder if args.host else DINOImageEncoder)(args.dino_dir)
        dino = DinoTerm(encoder, args.lambda_dino, args.dino_start_iter, os.path.join(args.model_path, "dino_loss_log.csv"))
    t0 = time.time()
    done = first_iter
    state = TrainState(seed=0)      # one view sampler for the whole run: saving does not perturb the trajectory
    for stop in sorted(set([i for i in args.save_iterations if first_iter < i <= args.iterations] + [args.iterations])):
        train(gaussians, scene.getTrainCameras(), opt, pipe, background, cameras_extent=scene.cameras_extent,
              first_iter=done, iterations=stop, view_parallel=vp, white_background=args.white_background,
              log_every=args.log_every if rank == 0 else 0, final_iteration=args.iterations, state=state, dino=dino)
        done = stop
        if vp is not None:
            vp.finish()
        if rank == 0:
            scene.save(stop)
            torch.save((gaussians.capture(), stop), os.path.join(args.model_path, f"chkpnt{stop}.pth"))
    if rank == 0:
        res = {"iterations": done, "seconds": time.time() - t0, "points": int(gaussians.get_xyz.shape[0]),
               "psnr_train": evaluate(gaussians, scene.getTrainCameras()[:8], pipe, background),
               "psnr_test": evaluate(gaussians, scene.getTestCameras(), pipe, background)}
        with open(os.path.join(args.model_path, "results.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
