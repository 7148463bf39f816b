"""Cull a mesh against the object masks of a DTU scan: the first half of the reference's
scripts/eval_dtu/evaluate_single_scene.py (cull_scan), with its arguments where they apply.

    python -m gaussmart_amd.cull_cli --input_mesh M.ply --scan_id 24 --mask_dir DIR --output_dir OUT [--radius 24] [--host]

reads DIR/scan24/cameras.npz and DIR/scan24/mask/*.png and writes OUT/culled_mesh.ply.  The Chamfer evaluation the reference
starts afterwards is not part of this command."""
import argparse
import os
import sys

from . import _lib
from .mesh import TriangleMesh
from .mesh_cull import DEFAULT_RADIUS, cull_mesh_by_masks, cull_mesh_by_masks_host, load_dtu_instance


def main(argv=None):
    ap = argparse.ArgumentParser(
        description="Remove the vertices of a mesh that some view of a DTU scan sees outside its dilated object mask.")
    ap.add_argument("--input_mesh", type=str, required=True, help="binary PLY to cull")
    ap.add_argument("--scan_id", type=str, required=True, help="DTU scan number: the scene is read from MASK_DIR/scan<id>")
    ap.add_argument("--output_dir", type=str, default="evaluation_results_single", help="directory that receives culled_mesh.ply")
    ap.add_argument("--mask_dir", type=str, default="mask", help="directory holding scan<id>/cameras.npz and scan<id>/mask/*.png")
    ap.add_argument("--radius", type=int, default=DEFAULT_RADIUS, help="radius of the dilation disk in pixels")
    ap.add_argument("--host", action="store_true", help="numpy + scipy instead of the device kernels")
    args = ap.parse_args(argv)
    try:
        if not os.path.isfile(args.input_mesh):
            raise FileNotFoundError(f"{args.input_mesh}: no such file")
        mesh = TriangleMesh.read_ply(args.input_mesh)
        inst = load_dtu_instance(os.path.join(args.mask_dir, f"scan{args.scan_id}"))
        if args.host:
            out = cull_mesh_by_masks_host(mesh, inst.proj, inst.masks, args.radius, scale=inst.scale, offset=inst.offset)
        else:
            import torch
            if not torch.cuda.is_available():
                raise _lib.GsrError("no GPU: the device path has no CPU fall-back (use --host)")
            out = cull_mesh_by_masks(mesh, inst.proj, inst.masks, args.radius, scale=inst.scale, offset=inst.offset,
                                     device=torch.device("cuda", 0)).cpu()
        path = os.path.join(args.output_dir, "culled_mesh.ply")
        out.write_ply(path)
    except (OSError, ValueError, _lib.GsrError) as e:
        print(f"cull_cli: {e}", file=sys.stderr)
        return 2
    print(f"num vertices raw {len(mesh.vertices)}, num triangles raw {len(mesh.triangles)}")
    print(f"num vertices culled {len(out.vertices)}, num triangles culled {len(out.triangles)}")
    print(f"wrote {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
