"""Step 2 of the reference's identification/main.py, the SAM masks of the chosen views, on the device.

    python -m gaussmart_amd.sam_cli -s SCAN -o OUT --views i j k ... --sam_checkpoint FILE_OR_DIR [--model_type vit_h|vit_l|vit_b] [--host]
        [--decoder torch|hip]
    python -m gaussmart_amd.sam_cli --sam2 -s SCAN -o OUT --views ... --sam_checkpoint DIR [--model_type large|base_plus|small|tiny] [--host]
        [--decoder torch|hip]
        [--points_per_side 32] [--pred_iou_thresh 0.86] [--stability_score_thresh 0.92]      (the reference's values)

View i is the i-th file of sorted(listdir(SCAN/images)).  Writes OUT/segments/masks/segments_NNN.npz (keys masks, boxes,
areas; the k-th file belongs to the k-th --views entry) and copies the images to OUT/segments/images/; prints one JSON line
per view.  `python -m gaussmart_amd.segment_cli --masks OUT/segments/masks --views ...` reads them.  --sam_checkpoint is a
LOCAL .pth under segment_anything's names or a LOCAL directory under transformers' (gaussmart_amd.sam.load_sam_weights);
nothing is downloaded.  --host runs transformers' encoder in fp32 and the torch selection on the same device.  --decoder hip
runs the prompt encoder and the mask decoder on the kernels of csrc/sam_decoder.hip (fp16 operands); torch, the default, runs
transformers' modules in fp32.
--sam2 is the reference's --sam2 branch (SAM2AutomaticMaskGenerator on sam2-hiera-large): the Hiera encoder and its neck on
the kernels of csrc/sam2.hip, the same files and JSON lines.  Its --sam_checkpoint is a LOCAL directory under transformers'
Sam2Model names (gaussmart_amd.sam2.load_sam2_weights).  --decoder hip runs SAM2's prompt encoder and mask decoder on the same
kernels of csrc/sam_decoder.hip (eight tokens per point, the two high-resolution skips, a sigmoid on the IoU head); with --host
it is refused, since --host runs the torch modules only.
The views come from the caller here; `python -m gaussmart_amd.identify_cli` picks them as the reference does (step 1, the camera
clustering of gaussmart_amd.camera_select) and runs steps 1 to 5 in one process.
Not built: crop layers, min_mask_region_area, and for SAM2 the object-score output, boxes and mask prompts, several points per
prompt and single-mask output.
"""
import argparse
import json
import os
import shutil
import sys

import numpy as np

from . import sam as S


def make_generator(args):
    """(generator, weights) for parsed arguments sam_checkpoint, sam2, model_type, host, decoder, device, points_per_side,
    pred_iou_thresh and stability_score_thresh (this command's and gaussmart_amd.identify_cli's)."""
    if args.model_type is not None and (args.model_type in ("vit_h", "vit_l", "vit_b")) == args.sam2:
        print(f"sam_cli: --model_type {args.model_type} does not go with {'--sam2' if args.sam2 else 'SAM (no --sam2)'}", file=sys.stderr)
        raise SystemExit(2)
    if args.sam2:
        from . import sam2 as S2
        weights = S2.load_sam2_weights(args.sam_checkpoint)
        if args.model_type is not None:
            want, have = S2.Sam2Config.preset(args.model_type), weights.config
            if (want.embed_dim, want.num_heads, tuple(want.blocks_per_stage)) != (have.embed_dim, have.num_heads, tuple(have.blocks_per_stage)):
                print(f"sam_cli: {args.sam_checkpoint} is not a {args.model_type} (embed {have.embed_dim}, blocks {tuple(have.blocks_per_stage)})",
                      file=sys.stderr)
                raise SystemExit(2)
    else:
        weights = S.load_sam_weights(args.sam_checkpoint)
        if args.model_type is not None:
            want, have = S.SamConfig.preset(args.model_type), weights.config
            if (want.hidden_size, want.num_hidden_layers, want.num_attention_heads) != (have.hidden_size, have.num_hidden_layers, have.num_attention_heads):
                print(f"sam_cli: {args.sam_checkpoint} is not a {args.model_type} (hidden {have.hidden_size}, {have.num_hidden_layers} layers)",
                      file=sys.stderr)
                raise SystemExit(2)
    gen = (S2.Sam2MaskGenerator if args.sam2 else S.SamMaskGenerator)(
        weights, points_per_side=args.points_per_side, pred_iou_thresh=args.pred_iou_thresh,
        stability_score_thresh=args.stability_score_thresh, host=args.host, device=args.device, decoder=args.decoder)
    return gen, weights


def main(argv=None):
    ap = argparse.ArgumentParser(prog="gaussmart_amd.sam_cli", description=__doc__.split("\n\n")[0])
    ap.add_argument("-s", "--scan_path", required=True)
    ap.add_argument("-o", "--output_path", required=True)
    ap.add_argument("--views", type=int, nargs="+", required=True, help="indices into sorted(listdir(SCAN/images))")
    ap.add_argument("--sam_checkpoint", required=True, help="a local .pth (segment_anything) or directory (transformers)")
    ap.add_argument("--sam2", action="store_true", help="SAM2 (Hiera) instead of SAM; --sam_checkpoint is then a local directory")
    ap.add_argument("--model_type", choices=("vit_h", "vit_l", "vit_b", "large", "base_plus", "small", "tiny"), default=None,
                    help="checked against the checkpoint's own shape when given (vit_*: SAM; the others: --sam2)")
    ap.add_argument("--host", action="store_true", help="transformers' encoder in fp32 and the torch selection")
    ap.add_argument("--decoder", choices=("torch", "hip"), default="torch", help="the prompt encoder and mask decoder: transformers' or the kernels")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--points_per_side", type=int, default=32)
    ap.add_argument("--pred_iou_thresh", type=float, default=0.86)
    ap.add_argument("--stability_score_thresh", type=float, default=0.92)
    args = ap.parse_args(argv)

    from PIL import Image
    image_dir = os.path.join(args.scan_path, "images")
    if not os.path.isdir(image_dir):
        print(f"sam_cli: {image_dir} is not a directory", file=sys.stderr)
        raise SystemExit(2)
    files = sorted(os.listdir(image_dir))
    bad = [i for i in args.views if not 0 <= i < len(files)]
    if bad:
        print(f"sam_cli: views {bad} are outside the {len(files)} images of {image_dir}", file=sys.stderr)
        raise SystemExit(2)
    gen, weights = make_generator(args)
    mask_dir = os.path.join(args.output_path, "segments", "masks")
    copy_dir = os.path.join(args.output_path, "segments", "images")
    os.makedirs(mask_dir, exist_ok=True)
    os.makedirs(copy_dir, exist_ok=True)
    for k, i in enumerate(args.views):
        path = os.path.join(image_dir, files[i])
        image = np.asarray(Image.open(path).convert("RGB"))
        masks = gen.generate(image)
        out = os.path.join(mask_dir, f"segments_{k:03d}.npz")
        if masks:
            S.save_segments_boxes(masks, out)
        else:               # the layout of an empty view: [0,h,w] masks
            e = gen.preprocess(image, weights.config.image_size)[2]
            np.savez(out, masks=np.zeros((0, *e), bool), boxes=np.zeros((0, 4), np.int64), areas=np.zeros((0,), np.int64))
        shutil.copy(path, os.path.join(copy_dir, files[i]))
        print(json.dumps({"view": i, "image": files[i], "masks": len(masks), "host": bool(args.host), "decoder": args.decoder,
                          **{f"{name}_ms": round(ms, 3) for name, ms in gen.last_ms.items()}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
