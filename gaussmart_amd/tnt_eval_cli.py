"""Score a mesh against a Tanks-and-Temples scan: the reference's scripts/eval_tnt/run.py, with its arguments.

    python -m gaussmart_amd.tnt_eval_cli --dataset-dir TNT_GT/Barn --traj-path Barn.log|poses.npy --ply-path M.ply
                                         [--out-dir OUT] [--tau T] [--init-transform FILE] [--host] [--write_vis]

The scene is the name of the dataset directory, which holds <scene>.ply, <scene>.json, <scene>_trans.txt and
<scene>_COLMAP_SfM.log; --tau overrides (or, for a scene this project has no entry for, supplies) the distance threshold.
The first alignment comes from the camera centres of --traj-path against the scene's COLMAP trajectory (align_trajectories),
or from --init-transform (a 4x4 text file).  Writes OUT/<scene>.precision.txt, .recall.txt and .prf_tau_plotstr.txt as the
reference does and OUT/results.json (precision, recall, fscore, tau, the final transformation, the three ICP traces); with
--write_vis also the two error-coloured clouds OUT/<scene>.precision.ply and .recall.ply (needs matplotlib for the colour
map).  OUT defaults to an `evaluation` directory beside the mesh.  No plot is drawn."""
import argparse
import json
import os
import sys

import numpy as np

from . import _lib
from . import tnt_eval as TE
from .mesh import TriangleMesh


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _read_poses(path):
    if path.endswith(".npy"):
        return np.asarray(np.load(path), np.float64).reshape(-1, 4, 4)
    if path.endswith(".log"):
        return TE.read_trajectory_log(path)
    raise ValueError(f"{path}: a trajectory is a .log or a .npy file")


def _write_vis(path, points, dist, max_distance):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        cmap = plt.get_cmap("hot_r")
    except ImportError:
        print(f"tnt_eval_cli: matplotlib is not installed, {path} is not written")
        return
    col = cmap(np.minimum(_host(dist), max_distance) / max_distance)[:, :3]
    TriangleMesh(_host(points), None, col).write_ply(path)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Precision, recall and F-score of a mesh against a Tanks-and-Temples scan.")
    ap.add_argument("--dataset-dir", type=str, required=True, help="the scene's directory: X.ply, X.json, X_trans.txt, X_COLMAP_SfM.log")
    ap.add_argument("--traj-path", type=str, required=True, help="the reconstruction's camera trajectory (.log or .npy of 4x4)")
    ap.add_argument("--ply-path", type=str, required=True, help="binary PLY: the (culled) mesh")
    ap.add_argument("--out-dir", type=str, default="")
    ap.add_argument("--tau", type=float, default=None, help="distance threshold in metres (default: the scene's)")
    ap.add_argument("--init-transform", type=str, default=None, help="4x4 text file: the first alignment, in place of the trajectories'")
    ap.add_argument("--host", action="store_true", help="numpy + scipy instead of the device kernels")
    ap.add_argument("--write_vis", action="store_true", help="also write the two error-coloured clouds")
    args = ap.parse_args(argv)
    try:
        scene = os.path.basename(os.path.normpath(args.dataset_dir))
        if args.tau is None and scene not in TE.SCENE_TAU:
            raise ValueError(f"no tau for scene {scene!r}: pass --tau, or use one of {', '.join(sorted(TE.SCENE_TAU))}")
        tau = float(args.tau) if args.tau is not None else TE.SCENE_TAU[scene]
        for f in (args.ply_path, args.traj_path) + ((args.init_transform,) if args.init_transform else ()):
            if not os.path.isfile(f):
                raise FileNotFoundError(f"{f}: no such file")
        inst = TE.load_tnt_instance(args.dataset_dir)
        mesh = TriangleMesh.read_ply(args.ply_path)
        if args.init_transform:
            init = np.loadtxt(args.init_transform).reshape(4, 4)
        else:
            init = TE.align_trajectories(TE.camera_centres(_read_poses(args.traj_path)), inst["gt_centres"])
        if args.host:
            res = TE.evaluate_tnt_mesh_host(mesh, inst["gt_points"], inst["crop"], tau, init)
        else:
            import torch
            if not torch.cuda.is_available():
                raise _lib.GsrError("no GPU: the device path has no CPU fall-back (use --host)")
            res = TE.evaluate_tnt_mesh(mesh, inst["gt_points"], inst["crop"], tau, init, device=torch.device("cuda", 0))
        out_dir = args.out_dir.strip() or os.path.join(os.path.dirname(args.ply_path), "evaluation")
        os.makedirs(out_dir, exist_ok=True)
        base = os.path.join(out_dir, scene)
        np.savetxt(base + ".recall.txt", res["cum_target"])
        np.savetxt(base + ".precision.txt", res["cum_source"])
        np.savetxt(base + ".prf_tau_plotstr.txt", np.array([res["precision"], res["recall"], res["fscore"], tau, res["stretch"]]))
        out = {"scene": scene, "precision": float(res["precision"]), "recall": float(res["recall"]), "fscore": float(res["fscore"]),
               "tau": tau, "transformation": np.asarray(res["transformation"]).tolist(),
               "icp": [{"fitness": r["fitness"], "inlier_rmse": r["inlier_rmse"], "iterations": r["iterations"],
                        "trace": [[int(c), float(e)] for c, e in r["trace"]]} for r in res["registrations"]]}
        with open(os.path.join(out_dir, "results.json"), "w") as f:
            json.dump(out, f, indent=True)
        if args.write_vis and res["dist_source"] is not None:
            _write_vis(base + ".precision.ply", res["cloud_source"], res["dist_source"], 3 * tau)
            _write_vis(base + ".recall.ply", res["cloud_target"], res["dist_target"], 3 * tau)
    except (OSError, ValueError, KeyError, _lib.GsrError) as e:
        print(f"tnt_eval_cli: {e}", file=sys.stderr)
        return 2
    print(out["precision"], out["recall"], out["fscore"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
