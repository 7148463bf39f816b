"""SAM automatic mask generation on the device: the reference's SAMSegmentation.process_image (identification/sam.py:41-46,
65-92: SamAutomaticMaskGenerator(vit_h, points_per_side=32, pred_iou_thresh=0.86, stability_score_thresh=0.92)) with the
image encoder and the mask selection computed by the kernels of csrc/sam.hip (include/gsr.h: SV_EMBED, SV_ATTN, SV_NECK,
SM_SCORE, SM_NMS, SM_EMIT).  The prompt encoder and the mask decoder are transformers' own torch modules, run on the device
in fp32 as they are (decoder="torch", the default), or the kernels of csrc/sam_decoder.hip (decoder="hip"; include/gsr.h:
SD_PROMPT, SD_IMAGE, SD_TOKENS, SD_T2I, SD_I2T, SD_UP, SD_HEADS: fp16 operands, fp32 accumulation and token stream).

    from gaussmart_amd.sam import SamMaskGenerator, load_sam_weights, save_segments_boxes
    gen = SamMaskGenerator(load_sam_weights("/models/sam_vit_h_4b8939.pth"))     # or a directory, see load_sam_weights
    masks = gen.generate(image_u8)                    # the reference's list of dicts, in NMS order
    save_segments_boxes(masks, "out/segments/masks/segments_000.npz")
    dev = gen.generate_device(image_u8)               # uint8 [m,h,w] on the device, what segment_init.label_points takes

What differs from the reference, on purpose:
  * nothing is fetched: `load_sam_weights` takes a LOCAL .pth (segment_anything's names) or a LOCAL directory (SamModel's).
  * the encoder's weights are fp16 and its matrix products take fp16 operands with fp32 accumulation; the residual stream,
    the LayerNorm statistics and the softmax are fp32.  The reference runs the encoder in fp32.
  * DEVIATION: the first resize (long side <= 1024) is cv2.INTER_LINEAR in the reference and PIL's bilinear here.
  * one full-image crop only: no crop layers, no min_mask_region_area.  The crop-edge filter of the reference never fires
    for the single full-image crop and is left out.  SAM2 (the reference's sam2=True) is gaussmart_amd/sam2.py.
`sam_host`, `decode_host`, `select_host` and `nms_host` are the torch twins (any device): they back `host=True` and the tests.
This module also holds what SAM2 shares, once: `ModelWeights`, `random_tensors`, `load_decoder`, `device_pixels`,
`grid_positional`, `decode_chunk`, and every step of `SamMaskGenerator`; sam2.py derives from these and supplies hooks only.
"""
import copy
import ctypes as C
import json
import math
import os
import re
import time
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._dev import ptr, stream, workspace

PATCH = 16
MASK_THRESHOLD = 0.0            # segment_anything's Sam.mask_threshold
IMAGE_MEAN = (123.675, 116.28, 103.53)
IMAGE_STD = (58.395, 57.12, 57.375)
MAX_SIDE = 1024                 # identification/sam.py:72
DECODER_CHANNELS = 256          # the stock prompt encoder and mask decoder

# the weight table of gsr_sam_encode, in the order of include/gsr.h (names under "vision_encoder.")
ENC_HEAD = ("patch_embed.projection.weight", "patch_embed.projection.bias", "pos_embed")
ENC_LAYER = ("layer_norm1.weight", "layer_norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.rel_pos_h", "attn.rel_pos_w",
             "attn.proj.weight", "attn.proj.bias", "layer_norm2.weight", "layer_norm2.bias", "mlp.lin1.weight", "mlp.lin1.bias",
             "mlp.lin2.weight", "mlp.lin2.bias")
ENC_NECK = ("neck.conv1.weight", "neck.layer_norm1.weight", "neck.layer_norm1.bias", "neck.conv2.weight",
            "neck.layer_norm2.weight", "neck.layer_norm2.bias")
assert (len(ENC_HEAD), len(ENC_LAYER), len(ENC_NECK)) == (_lib.GSR_SAM_W_LAYER0, _lib.GSR_SAM_W_PER_LAYER, _lib.GSR_SAM_W_NECK)
VISION = "vision_encoder."

# the weight table of gsr_sam_decode, in the order of include/gsr.h (names of SamModel.state_dict())
_ATTN = tuple(f"{p}_proj.{x}" for p in ("q", "k", "v", "out") for x in ("weight", "bias"))
_NORM = ("weight", "bias")
DEC_HEAD = ("prompt_encoder.shared_embedding.positional_embedding", "prompt_encoder.point_embed.1.weight",
            "prompt_encoder.not_a_point_embed.weight", "prompt_encoder.no_mask_embed.weight", "mask_decoder.iou_token.weight",
            "mask_decoder.mask_tokens.weight")
DEC_LAYER = (tuple(f"self_attn.{k}" for k in _ATTN) + tuple(f"layer_norm1.{k}" for k in _NORM)
             + tuple(f"cross_attn_token_to_image.{k}" for k in _ATTN) + tuple(f"layer_norm2.{k}" for k in _NORM)
             + ("mlp.lin1.weight", "mlp.lin1.bias", "mlp.lin2.weight", "mlp.lin2.bias") + tuple(f"layer_norm3.{k}" for k in _NORM)
             + tuple(f"layer_norm4.{k}" for k in _NORM) + tuple(f"cross_attn_image_to_token.{k}" for k in _ATTN))
DEC_FINAL = tuple(f"final_attn_token_to_image.{k}" for k in _ATTN) + tuple(f"layer_norm_final_attn.{k}" for k in _NORM)
DEC_UP = ("upscale_conv1.weight", "upscale_conv1.bias", "upscale_layer_norm.weight", "upscale_layer_norm.bias", "upscale_conv2.weight",
          "upscale_conv2.bias")
_MLP3 = tuple(f"{p}.{x}" for p in ("proj_in", "layers.0", "proj_out") for x in ("weight", "bias"))
DEC_HYPER = tuple(f"output_hypernetworks_mlps.{m}.{k}" for m in (1, 2, 3) for k in _MLP3)
DEC_IOU = tuple(f"iou_prediction_head.{k}" for k in _MLP3)
DEC_LAYERS = 2
assert (len(DEC_HEAD), len(DEC_LAYER)) == (_lib.GSR_SAMD_W_LAYER0, _lib.GSR_SAMD_W_PER_LAYER)
assert _lib.GSR_SAMD_W_FINAL == len(DEC_HEAD) + DEC_LAYERS * len(DEC_LAYER) and _lib.GSR_SAMD_W_UP == _lib.GSR_SAMD_W_FINAL + len(DEC_FINAL)
assert _lib.GSR_SAMD_W_HYPER == _lib.GSR_SAMD_W_UP + len(DEC_UP) and _lib.GSR_SAMD_W_IOU == _lib.GSR_SAMD_W_HYPER + len(DEC_HYPER)
assert _lib.GSR_SAMD_W_COUNT == _lib.GSR_SAMD_W_IOU + len(DEC_IOU)
DECODER_WORKSPACE_BUDGET = 2 << 30       # bytes of gsr_sam_decode workspace per call of decoder="hip": the points are chunked to fit
TIED = ("prompt_encoder.shared_embedding.positional_embedding", "shared_image_embedding.positional_embedding")


@dataclass
class SamConfig:
    """Defaults: ViT-H (sam_vit_h_4b8939), what the reference loads."""
    hidden_size: int = 1280
    num_hidden_layers: int = 32
    num_attention_heads: int = 16
    mlp_dim: int = 5120
    window_size: int = 14
    global_attn_indexes: tuple = (7, 15, 23, 31)
    output_channels: int = 256
    image_size: int = 1024
    layer_norm_eps: float = 1e-6

    @classmethod
    def preset(cls, model_type):
        if model_type == "vit_h":
            return cls()
        if model_type == "vit_l":
            return cls(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, mlp_dim=4096, global_attn_indexes=(5, 11, 17, 23))
        if model_type == "vit_b":
            return cls(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_dim=3072, global_attn_indexes=(2, 5, 8, 11))
        raise ValueError(f"sam: model_type {model_type!r} is not vit_h, vit_l or vit_b")

    @property
    def grid(self):
        return self.image_size // PATCH

    @property
    def head_dim(self):
        return self.hidden_size // max(1, self.num_attention_heads)

    def windows(self):
        """Per layer: 0 for a global layer, else the window size."""
        return [0 if l in tuple(self.global_attn_indexes) else int(self.window_size) for l in range(self.num_hidden_layers)]

    def to_hf(self):
        from transformers import SamConfig as HfSam, SamVisionConfig, SamPromptEncoderConfig, SamMaskDecoderConfig
        vision = SamVisionConfig(hidden_size=self.hidden_size, output_channels=self.output_channels,
                                 num_hidden_layers=self.num_hidden_layers, num_attention_heads=self.num_attention_heads,
                                 image_size=self.image_size, patch_size=PATCH, layer_norm_eps=self.layer_norm_eps,
                                 window_size=self.window_size, global_attn_indexes=list(self.global_attn_indexes), mlp_dim=self.mlp_dim)
        hf = HfSam(vision_config=vision, prompt_encoder_config=SamPromptEncoderConfig(image_size=self.image_size),
                   mask_decoder_config=SamMaskDecoderConfig())
        hf.vision_config._attn_implementation = "eager"
        hf.mask_decoder_config._attn_implementation = "eager"
        return hf

    def to_json(self):
        return {"model_type": "sam", "vision_config": {
            "hidden_size": self.hidden_size, "num_hidden_layers": self.num_hidden_layers, "num_attention_heads": self.num_attention_heads,
            "mlp_dim": self.mlp_dim, "window_size": self.window_size, "global_attn_indexes": list(self.global_attn_indexes),
            "output_channels": self.output_channels, "image_size": self.image_size, "layer_norm_eps": self.layer_norm_eps,
            "patch_size": PATCH}}

    @classmethod
    def from_json(cls, d):
        v = d.get("vision_config", d)
        if v.get("patch_size", PATCH) != PATCH:
            raise NotImplementedError(f"sam: patch size {v['patch_size']} is not built (16 only)")
        hidden = int(v.get("hidden_size", 768))
        mlp = v.get("mlp_dim") or int(hidden * v.get("mlp_ratio", 4.0))
        return cls(hidden_size=hidden, num_hidden_layers=int(v.get("num_hidden_layers", 12)),
                   num_attention_heads=int(v.get("num_attention_heads", 12)), mlp_dim=int(mlp), window_size=int(v.get("window_size", 14)),
                   global_attn_indexes=tuple(v.get("global_attn_indexes", (2, 5, 8, 11))), output_channels=int(v.get("output_channels", 256)),
                   image_size=int(v.get("image_size", 1024)), layer_norm_eps=float(v.get("layer_norm_eps", 1e-6)))


def model_shapes(config, model="SamModel"):
    """name -> shape of the state_dict() of transformers' `model` for this configuration (built on the meta device)."""
    import transformers
    with torch.device("meta"):
        sd = getattr(transformers, model)(config.to_hf()).state_dict()
    return {k: tuple(v.shape) for k, v in sd.items()}


class ModelWeights:
    """What SamWeights and Sam2Weights share: config + the tensors under the names of a transformers model's state_dict(),
    validated against its shapes, the vision encoder in fp16 (what the kernels take) and the rest in fp32; `copy`, `to`, `sub`
    and the weight table of the decoder kernels.  A subclass sets the class attributes below and adds its encoder's table()."""
    WHO, MODEL = None, None             # the prefix of every message; transformers' class whose state_dict() names the tensors
    IGNORED = ()                        # patterns of keys that are dropped unread
    HALF = ()                           # keys outside the vision encoder that are kept in fp16 too
    # the decoder's weight table: the names of its head, of one layer, of the final attention and of what follows the IoU head,
    # and the rows of the point_embed tensor (slot GSR_SAMD_W_POINT1) that the table takes
    DEC_HEAD, DEC_LAYER, DEC_FINAL, DEC_TAIL, POINT_ROWS = (), (), (), (), slice(None)

    def __init__(self, config, tensors, decoder=True):
        who = self.WHO
        self.config, self.decoder, self.tensors = config, bool(decoder), {}
        tensors = {k: v for k, v in dict(tensors).items() if not any(re.search(p, k) for p in self.IGNORED)}
        for a, b in (TIED, TIED[::-1]):
            if decoder and a not in tensors and b in tensors:
                tensors[a] = tensors[b]
        want = {k: s for k, s in model_shapes(config, self.MODEL).items() if decoder or k.startswith(VISION)}
        unknown = sorted(set(tensors) - set(want))
        if unknown:
            raise KeyError(f"{who} weights: {len(unknown)} tensors have no place, e.g. {unknown[:3]}")
        missing = sorted(set(want) - set(tensors))
        if missing:
            raise KeyError(f"{who} weights: {len(missing)} tensors are not filled, e.g. {missing[:3]}")
        for k, shape in want.items():
            t = tensors[k].detach()
            if tuple(t.shape) != shape:
                raise ValueError(f"{who} weights: {k} must be {list(shape)}, got {list(t.shape)}")
            self.tensors[k] = t.to(torch.float16 if k.startswith(VISION) or k in self.HALF else torch.float32).contiguous()

    def copy(self, replace=None, keep=None, device=None):
        """A copy that shares the configuration: the tensors of `replace` (name -> tensor) in place of these, only the names
        `keep(name)` accepts, all on `device` (None: where they are).  Neither this object nor its dict is changed."""
        w = copy.copy(self)
        w.tensors = {k: t if device is None else t.to(device) for k, t in {**self.tensors, **(replace or {})}.items()
                     if keep is None or keep(k)}
        return w

    def to(self, device):
        return self.copy(device=device)

    def decoder_table(self):
        """The tensors of the weight table of gsr_sam_decode (gsr_sam2_decode for Sam2Weights), in its order, on the tensors'
        device: fp16 copies (self.tensors keeps its fp32 ones), except the positional matrix (fp32, as it is).  The two
        transposed convolutions [ci,co,2,2] are re-laid as [(dy 2 + dx) co_n + co][ci] and their biases repeated per tap, which
        is what one DN_LINEAR over the input channels takes."""
        if not self.decoder:
            raise ValueError(f"{self.WHO}: these weights hold no prompt encoder and mask decoder")
        t, md = self.tensors, "mask_decoder."
        names = list(self.DEC_HEAD)
        for l in range(DEC_LAYERS):
            names += [f"{md}transformer.layers.{l}.{k}" for k in self.DEC_LAYER]
        names += [f"{md}transformer.{k}" for k in self.DEC_FINAL] + [md + k for k in DEC_UP + DEC_HYPER + DEC_IOU] + list(self.DEC_TAIL)
        out = []
        for k in names:
            v = t[k]
            if k == names[0]:
                out.append(v.to(torch.float32).contiguous())
                continue
            if k == names[_lib.GSR_SAMD_W_POINT1]:
                v = v[self.POINT_ROWS]
            elif k.startswith(md + "upscale_conv") and k.endswith(".weight"):
                v = v.permute(2, 3, 1, 0).reshape(4 * v.shape[1], v.shape[0])
            elif k.startswith(md + "upscale_conv"):
                v = v.repeat(4)
            out.append(v.to(torch.float16).contiguous())
        assert len(out) == _lib.GSR_SAMD_W_COUNT + len(self.DEC_TAIL)
        return out

    def sub(self, prefix):
        """The tensors under `prefix`, with it removed (a sub-module's state dict), in fp32."""
        return {k[len(prefix):]: t.to(torch.float32) for k, t in self.tensors.items() if k.startswith(prefix)}


class SamWeights(ModelWeights):
    """config + the tensors under SamModel.state_dict()'s names: the vision encoder in fp16 (what the kernels take), the
    prompt encoder, the mask decoder and the shared positional embedding in fp32.  decoder=False: the vision encoder alone
    (any output_channels; the stock decoder needs 256)."""
    WHO, MODEL = "sam", "SamModel"
    DEC_HEAD, DEC_LAYER, DEC_FINAL = DEC_HEAD, DEC_LAYER, DEC_FINAL

    def __init__(self, config, tensors, decoder=True):
        if decoder and config.output_channels != DECODER_CHANNELS:
            raise ValueError(f"sam weights: the decoder needs {DECODER_CHANNELS} output channels, the encoder has {config.output_channels}")
        super().__init__(config, tensors, decoder)

    def table(self):
        """The vision encoder's tensors in the order of gsr_sam_encode's weight table."""
        names = [VISION + k for k in ENC_HEAD]
        for l in range(self.config.num_hidden_layers):
            names += [f"{VISION}layers.{l}.{k}" for k in ENC_LAYER]
        return [self.tensors[k] for k in names + [VISION + k for k in ENC_NECK]]


# ---------------------------------------------------------------- segment_anything's names <-> SamModel's
_NECK = {"0": "conv1", "1": "layer_norm1", "2": "conv2", "3": "layer_norm2"}
_DOWN = {"0": "conv1", "1": "layer_norm1", "3": "conv2", "4": "layer_norm2", "6": "conv3"}
_UP = {"0": "upscale_conv1", "1": "upscale_layer_norm", "3": "upscale_conv2"}
_MLP = {"0": "proj_in", "1": "layers.0", "2": "proj_out"}
_GAUSS = "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"


def _inv(d):
    return {v: k for k, v in d.items()}


def pth_to_hf(name):
    """A key of segment_anything's Sam.state_dict() -> the key of transformers' SamModel.state_dict(); None: no place."""
    if name == _GAUSS:
        return TIED[1]
    if name.startswith("image_encoder."):
        k = name[len("image_encoder."):]
        k = re.sub(r"^blocks\.(\d+)\.norm([12])\.", r"layers.\1.layer_norm\2.", k)
        k = re.sub(r"^blocks\.", "layers.", k)
        k = re.sub(r"^patch_embed\.proj\.", "patch_embed.projection.", k)
        m = re.match(r"^neck\.(\d)\.(.*)$", k)
        if m:
            if m.group(1) not in _NECK:
                return None
            k = f"neck.{_NECK[m.group(1)]}.{m.group(2)}"
        return VISION + k
    if name.startswith("prompt_encoder."):
        k = name[len("prompt_encoder."):]
        k = re.sub(r"^point_embeddings\.", "point_embed.", k)
        m = re.match(r"^mask_downscaling\.(\d)\.(.*)$", k)
        if m:
            if m.group(1) not in _DOWN:
                return None
            k = f"mask_embed.{_DOWN[m.group(1)]}.{m.group(2)}"
        return "prompt_encoder." + k
    if name.startswith("mask_decoder."):
        k = name[len("mask_decoder."):]
        k = re.sub(r"^(transformer\.layers\.\d+)\.norm([1-4])\.", r"\1.layer_norm\2.", k)
        k = re.sub(r"^transformer\.norm_final_attn\.", "transformer.layer_norm_final_attn.", k)
        m = re.match(r"^output_upscaling\.(\d)\.(.*)$", k)
        if m:
            if m.group(1) not in _UP:
                return None
            k = f"{_UP[m.group(1)]}.{m.group(2)}"
        m = re.match(r"^(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.layers\.(\d)\.(.*)$", k)
        if m:
            if m.group(2) not in _MLP:
                return None
            k = f"{m.group(1)}.{_MLP[m.group(2)]}.{m.group(3)}"
        return "mask_decoder." + k
    return None


def hf_to_pth(name):
    """The inverse of pth_to_hf (the tied copy of the positional embedding has no key of its own: None)."""
    if name == TIED[1]:
        return _GAUSS
    if name == TIED[0]:
        return None
    if name.startswith(VISION):
        k = name[len(VISION):]
        k = re.sub(r"^layers\.(\d+)\.layer_norm([12])\.", r"blocks.\1.norm\2.", k)
        k = re.sub(r"^layers\.", "blocks.", k)
        k = re.sub(r"^patch_embed\.projection\.", "patch_embed.proj.", k)
        m = re.match(r"^neck\.(conv1|layer_norm1|conv2|layer_norm2)\.(.*)$", k)
        if m:
            k = f"neck.{_inv(_NECK)[m.group(1)]}.{m.group(2)}"
        return "image_encoder." + k
    if name.startswith("prompt_encoder."):
        k = name[len("prompt_encoder."):]
        k = re.sub(r"^point_embed\.", "point_embeddings.", k)
        m = re.match(r"^mask_embed\.(\w+)\.(.*)$", k)
        if m:
            k = f"mask_downscaling.{_inv(_DOWN)[m.group(1)]}.{m.group(2)}"
        return "prompt_encoder." + k
    if name.startswith("mask_decoder."):
        k = name[len("mask_decoder."):]
        k = re.sub(r"^(transformer\.layers\.\d+)\.layer_norm([1-4])\.", r"\1.norm\2.", k)
        k = re.sub(r"^transformer\.layer_norm_final_attn\.", "transformer.norm_final_attn.", k)
        m = re.match(r"^(upscale_conv1|upscale_layer_norm|upscale_conv2)\.(.*)$", k)
        if m:
            k = f"output_upscaling.{_inv(_UP)[m.group(1)]}.{m.group(2)}"
        m = re.match(r"^(output_hypernetworks_mlps\.\d+|iou_prediction_head)\.(proj_in|layers\.0|proj_out)\.(.*)$", k)
        if m:
            k = f"{m.group(1)}.layers.{_inv(_MLP)[m.group(2)]}.{m.group(3)}"
        return "mask_decoder." + k
    return None


def _config_from_pth(sd):
    """The encoder's shape read off the tensors of a segment_anything checkpoint."""
    pos = sd["image_encoder.pos_embed"]
    g, hidden = int(pos.shape[1]), int(pos.shape[3])
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("image_encoder.blocks."))
    head_dim = int(sd["image_encoder.blocks.0.attn.rel_pos_h"].shape[1])
    rows = [int(sd[f"image_encoder.blocks.{l}.attn.rel_pos_h"].shape[0]) for l in range(layers)]
    glob = tuple(l for l in range(layers) if rows[l] == 2 * g - 1)
    win = [(r + 1) // 2 for l, r in enumerate(rows) if l not in glob]
    return SamConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=hidden // head_dim,
                     mlp_dim=int(sd["image_encoder.blocks.0.mlp.lin1.weight"].shape[0]), window_size=win[0] if win else g,
                     global_attn_indexes=glob, output_channels=int(sd["image_encoder.neck.0.weight"].shape[0]), image_size=PATCH * g)


def load_sam_weights(path):
    """A LOCAL directory with config.json and model.safetensors under SamModel's names, or a LOCAL .pth under
    segment_anything's Sam.state_dict() names (identification/weights/sam_vit_h_4b8939.pth).  Nothing here opens a URL.
    Raises on any key it cannot place and on any key left unfilled."""
    path = os.fspath(path)
    if os.path.isdir(path):
        with open(os.path.join(path, "config.json")) as f:
            cfg = SamConfig.from_json(json.load(f))
        from safetensors.torch import load_file
        return SamWeights(cfg, load_file(os.path.join(path, "model.safetensors"), device="cpu"))
    if not os.path.isfile(path):
        raise FileNotFoundError(f"sam: {path!r} is neither a local directory nor a local .pth file.  The weights are never downloaded")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    tensors = {}
    for k, v in sd.items():
        name = pth_to_hf(k)
        if name is None:
            raise KeyError(f"sam weights: {k} of {path} has no place in SamModel")
        tensors[name] = v
    return SamWeights(_config_from_pth(sd), tensors)


def save_sam_weights(weights, directory):
    """Writes what load_sam_weights reads from a directory (config.json, model.safetensors)."""
    from safetensors.torch import save_file
    if not weights.decoder:
        raise ValueError("sam: only weights with a decoder can be saved")
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(weights.config.to_json(), f, indent=1)
    save_file({k: t.cpu().clone().contiguous() for k, t in weights.tensors.items()}, os.path.join(directory, "model.safetensors"))


def random_sam_weights(config=None, seed=0, decoder=None):
    """Seeded stand-ins at a scale where every part of the network shows in the output: linear, convolution and patch
    weights N(0, 1/fan_in), pos_embed and the embeddings N(0, 1), relative-position tables N(0, 1/head_dim), LayerNorm gains
    U(0.5, 1.5), biases N(0, 0.1^2), everything rounded to fp16.  decoder: default, whenever the encoder has 256 channels."""
    cfg = config or SamConfig()
    decoder = cfg.output_channels == DECODER_CHANNELS if decoder is None else decoder
    return SamWeights(cfg, random_tensors(model_shapes(cfg), seed, lambda k: decoder or k.startswith(VISION), rel_pos=math.sqrt(cfg.head_dim)),
                      decoder=decoder)


def random_tensors(shapes, seed, keep=None, unit=(), rel_pos=None):
    """The recipe of random_sam_weights and random_sam2_weights: one draw per tensor of `shapes`, in its order, from one generator
    (the tied copy of the positional matrix and the names `keep` refuses draw nothing).  unit: further names drawn N(0, 1);
    rel_pos: what the N(0, 1) draws of SAM's relative-position tables are divided by."""
    g = torch.Generator().manual_seed(seed)
    tensors = {}
    for name, shape in shapes.items():
        if name == TIED[0] or keep is not None and not keep(name):
            continue
        if rel_pos is not None and "rel_pos_" in name:
            t = torch.randn(shape, generator=g) / rel_pos
        elif "pos_embed" in name or name.endswith("positional_embedding") or name in unit or len(shape) == 2 and shape[0] <= 8 and "embed" in name \
                or name.endswith("_token.weight") or name.endswith("_tokens.weight"):
            t = torch.randn(shape, generator=g)
        elif "norm" in name and name.endswith(".weight"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
        tensors[name] = t.to(torch.float16)
    return tensors


# ---------------------------------------------------------------- the twin
def host_encoder(weights, dtype=torch.float64, device="cpu"):
    """transformers' SamVisionEncoder holding these tensors, in `dtype` on `device`, in eval mode."""
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    model = SamVisionEncoder(weights.config.to_hf().vision_config)
    model.load_state_dict(weights.sub(VISION), strict=True)
    return model.to(device=device, dtype=dtype).eval()


@torch.no_grad()
def sam_host(weights, pixel_values, dtype=torch.float64, device=None, model=None):
    """[C,g,g] of pixel_values [3,S,S] through the library's own encoder."""
    device = pixel_values.device if device is None else device
    model = host_encoder(weights, dtype, device) if model is None else model
    x = pixel_values.reshape(1, 3, *pixel_values.shape[-2:]).to(device=device, dtype=dtype)
    return model(x).last_hidden_state[0]


def host_decoder(weights, dtype=torch.float32, device="cpu"):
    """(SamPromptEncoder, SamMaskDecoder, wide [1,256,g,g]) holding these tensors, in `dtype` on `device`, in eval mode; wide
    is SamModel.get_image_wide_positional_embeddings()."""
    from transformers.models.sam.modeling_sam import SamPromptEncoder, SamMaskDecoder, SamPositionalEmbedding
    hf = weights.config.to_hf()
    return load_decoder(weights, (SamPromptEncoder(hf), SamMaskDecoder(hf.mask_decoder_config), SamPositionalEmbedding(hf.vision_config)),
                        weights.config.grid, dtype, device)


def load_decoder(weights, modules, g, dtype, device):
    """host_decoder's and host_decoder2's common part: modules = fresh (prompt encoder, mask decoder, shared positional
    embedding) -> (prompt, decoder, wide [1,256,g,g]) holding the tensors of `weights`, in `dtype` on `device`, in eval mode."""
    for m, prefix in zip(modules, ("prompt_encoder.", "mask_decoder.", "shared_image_embedding.")):
        m.load_state_dict(weights.sub(prefix), strict=True)
    prompt, decoder, shared = (m.to(device=device, dtype=dtype).eval() for m in modules)
    c = (torch.arange(g, device=device, dtype=dtype) + 0.5) / g      # get_image_wide_positional_embeddings
    with torch.no_grad():
        wide = shared(torch.stack([c[None, :].expand(g, g), c[:, None].expand(g, g)], -1)).permute(2, 0, 1)[None]
    return prompt, decoder, wide


@torch.no_grad()
def decode_host(weights, emb, wide, points, dtype=torch.float32, device=None, modules=None, points_per_batch=64):
    """transformers' prompt encoder and mask decoder as they are: emb [1,256,g,g], points [P,2] (x, y) in the input frame, one
    foreground point per prompt, multimask output -> (low_res [P,3,4g,4g], iou [P,3]) in `dtype`.  wide=None: computed here;
    modules: what host_decoder returned (built here otherwise)."""
    device = emb.device if device is None else torch.device(device)
    prompt, decoder, own = host_decoder(weights, dtype, device) if modules is None else modules
    wide = own if wide is None else wide.to(device=device, dtype=dtype)
    emb = emb.to(device=device, dtype=dtype)
    low, iou = [], []
    for part in points.to(device=device, dtype=torch.float64 if dtype == torch.float64 else torch.float32).split(points_per_batch):
        pts = part[None, :, None, :]
        labels = torch.ones(1, part.shape[0], 1, dtype=torch.int64, device=device)
        sparse, dense = prompt(pts, labels, None, None)
        m, q = decoder(image_embeddings=emb, image_positional_embeddings=wide, sparse_prompt_embeddings=sparse.to(dtype),
                       dense_prompt_embeddings=dense, multimask_output=True)
        low.append(m[0])
        iou.append(q[0])
    return torch.cat(low).contiguous(), torch.cat(iou).contiguous()


# ---------------------------------------------------------------- the encoder
def device_pixels(who, pixel_values, S):
    """The input check of both encoders' encode(): -> f32 [3,S,S], contiguous, on the device it came on."""
    if not isinstance(pixel_values, torch.Tensor) or not pixel_values.is_cuda:
        raise _lib.GsrError(f"{who}: pixel_values must live on the device (no CPU path; see {who}_host)")
    x = pixel_values.detach().reshape(-1, S, S) if pixel_values.numel() == 3 * S * S else pixel_values
    if tuple(x.shape) != (3, S, S):
        raise ValueError(f"{who}: expected [3,{S},{S}], got {list(pixel_values.shape)}")
    return x.to(torch.float32).contiguous()


class SamImageEncoder:
    """encode(pixel_values f32 [3,S,S] on the device) -> f32 [C,g,g], on the kernels."""

    def __init__(self, weights):
        self.weights, self.config = weights, weights.config
        self._on = {}

    def _device(self, dev):
        hit = self._on.get(dev)
        if hit is None:
            cfg = self.config
            w = self.weights.to(dev)
            tensors = w.table()
            table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            windows = (C.c_int32 * cfg.num_hidden_layers)(*cfg.windows())
            rows = (C.c_int32 * cfg.num_hidden_layers)(*[int(w.tensors[f"{VISION}layers.{l}.attn.rel_pos_h"].shape[0])
                                                         for l in range(cfg.num_hidden_layers)])
            for l in range(cfg.num_hidden_layers):
                a, b = (w.tensors[f"{VISION}layers.{l}.attn.rel_pos_{x}"] for x in "hw")
                if a.shape != b.shape:
                    raise ValueError(f"sam: rel_pos_h and rel_pos_w of layer {l} differ in shape")
            c = _lib.GsrSamConfig(cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.num_hidden_layers, cfg.mlp_dim,
                                  cfg.output_channels, cfg.image_size, cfg.layer_norm_eps, windows, rows)
            L = _lib.lib()
            nbytes = L.gsr_sam_workspace_bytes(C.byref(c))
            hit = self._on[dev] = dict(w=w, table=table, n=len(tensors), cfg=c, keep=(windows, rows), nbytes=nbytes,
                                       ws=workspace(nbytes, dev) if nbytes else None)
        return hit

    @torch.no_grad()
    def encode(self, pixel_values):
        cfg = self.config
        x = device_pixels("sam", pixel_values, cfg.image_size)
        dev = x.device
        d = self._device(dev)
        out = torch.empty(cfg.output_channels, cfg.grid, cfg.grid, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gsr_sam_encode(C.byref(d["cfg"]), d["table"], d["n"], ptr(x), ptr(d["ws"]), d["nbytes"], ptr(out),
                                             stream(dev)))
        return out


def preprocess(image_u8, image_size=1024):
    """HxWx3 uint8 -> (pixel_values f32 [3,S,S] on the host, input_size (ih, iw), mask_size (oh, ow)).  The reference's
    resize to a long side <= 1024 (identification/sam.py:71-76; mask_size is that picture's size, which the masks come out
    at), ResizeLongestSide to `image_size`, normalisation, then zero padding."""
    from PIL import Image
    img = Image.fromarray(np.ascontiguousarray(image_u8, np.uint8)[..., :3])
    w, h = img.size
    if max(h, w) > MAX_SIDE:
        scale = MAX_SIDE / max(h, w)
        img = img.resize((int(w * scale), int(h * scale)), Image.BILINEAR)
    ow, oh = img.size
    scale = image_size * 1.0 / max(oh, ow)
    ih, iw = int(oh * scale + 0.5), int(ow * scale + 0.5)
    if (ih, iw) != (oh, ow):
        img = img.resize((iw, ih), Image.BILINEAR)
    x = torch.from_numpy(np.asarray(img, np.uint8).copy()).permute(2, 0, 1).to(torch.float32)
    x = (x - torch.tensor(IMAGE_MEAN).view(3, 1, 1)) / torch.tensor(IMAGE_STD).view(3, 1, 1)
    out = torch.zeros(3, image_size, image_size, dtype=torch.float32)
    out[:, :ih, :iw] = x
    return out, (ih, iw), (oh, ow)


def point_grid(n, input_size):
    """f32 [n n,2] (x, y): ((i + 0.5) / n, (j + 0.5) / n) with x fastest, scaled to the input frame (ih, iw)."""
    c = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    xy = torch.stack([c[None, :].expand(n, n), c[:, None].expand(n, n)], -1).reshape(-1, 2)
    return (xy * torch.tensor([input_size[1], input_size[0]], dtype=torch.float64)).to(torch.float32)


# ---------------------------------------------------------------- selection: the torch twins
def nms_host(boxes, scores, keep_in, theta):
    """SM_NMS in torch: -> int64 indices of the kept boxes, by score descending (ties by index ascending)."""
    boxes, scores = boxes.to(torch.float32), scores.to(torch.float32)
    cand = torch.ones_like(scores, dtype=torch.bool) if keep_in is None else keep_in.to(torch.bool)
    cand = cand & ~torch.isnan(scores)
    idx = torch.nonzero(cand).reshape(-1)
    idx = idx[torch.sort(scores[idx], descending=True, stable=True).indices]
    b = boxes[idx]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = torch.zeros(len(idx), dtype=torch.bool, device=boxes.device)
    kept = []
    for i in range(len(idx)):
        if dead[i]:
            continue
        kept.append(int(idx[i]))
        w = (torch.minimum(b[i, 2], b[i + 1:, 2]) - torch.maximum(b[i, 0], b[i + 1:, 0])).clamp(min=0)
        h = (torch.minimum(b[i, 3], b[i + 1:, 3]) - torch.maximum(b[i, 1], b[i + 1:, 1])).clamp(min=0)
        inter = w * h
        dead[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > theta
    return torch.tensor(kept, dtype=torch.int64, device=boxes.device)


def upsample_host(logits, input_size, mask_size, dtype=None, direct=False):
    """[n,L,L] -> [n,oh,ow]: F.interpolate(L -> 4 L), the crop to input_size, F.interpolate to mask_size (bilinear,
    align_corners=False), in `dtype` (default: the logits' own).  direct: SAM2's one F.interpolate from L x L to mask_size
    (input_size is not read)."""
    x = logits.to(dtype or logits.dtype)[:, None]
    if direct:
        return F.interpolate(x, tuple(mask_size), mode="bilinear", align_corners=False)[:, 0]
    S = 4 * logits.shape[-1]
    x = F.interpolate(x, (S, S), mode="bilinear", align_corners=False)[..., :input_size[0], :input_size[1]]
    return F.interpolate(x, tuple(mask_size), mode="bilinear", align_corners=False)[:, 0]


def mask_stats_host(values, tau=MASK_THRESHOLD, delta=1.0):
    """(area, inter, union int64 [n], boxes f32 [n,4] inclusive XYXY, zeros when empty) of planes [n,h,w]."""
    on = values > tau
    area, inter, union = on.flatten(1).sum(1), (values > tau + delta).flatten(1).sum(1), (values > tau - delta).flatten(1).sum(1)
    n, h, w = on.shape
    cols, rows = on.any(1), on.any(2)
    big = max(h, w)
    xs, ys = torch.arange(w, device=on.device), torch.arange(h, device=on.device)
    x0, x1 = torch.where(cols, xs, big).min(1).values, torch.where(cols, xs, -1).max(1).values
    y0, y1 = torch.where(rows, ys, big).min(1).values, torch.where(rows, ys, -1).max(1).values
    boxes = torch.stack([x0, y0, x1, y1], 1).to(torch.float32)
    boxes[area == 0] = 0
    return area, inter, union, boxes


def select_host(low_res, iou, input_size, mask_size, pred_iou_thresh=0.86, stability_score_thresh=0.92, stability_score_offset=1.0,
                box_nms_thresh=0.7, dtype=None, chunk=64, direct=False):
    """SamMaskGenerator.select in torch (any device): the same gates in the same order on up-sampled planes.  direct: SAM2's
    one-step resampling (Sam2MaskGenerator.select)."""
    L = low_res.shape[-1]
    logits, scores = low_res.reshape(-1, L, L), iou.reshape(-1).to(torch.float32)
    n = logits.shape[0]
    first = scores > pred_iou_thresh
    area, inter, union = (torch.zeros(n, dtype=torch.int64, device=logits.device) for _ in range(3))
    boxes = torch.zeros(n, 4, dtype=torch.float32, device=logits.device)
    todo = torch.nonzero(first).reshape(-1)
    for part in todo.split(chunk):
        a, i, u, b = mask_stats_host(upsample_host(logits[part], input_size, mask_size, dtype, direct), MASK_THRESHOLD, stability_score_offset)
        area[part], inter[part], union[part], boxes[part] = a, i, u, b
    stab = inter.to(torch.float32) / union.to(torch.float32)
    keep_in = first & (stab >= stability_score_thresh)            # 0 / 0 is NaN and fails
    index = nms_host(boxes, scores, keep_in, box_nms_thresh)
    masks = torch.zeros(len(index), *mask_size, dtype=torch.uint8, device=logits.device)
    for part in torch.arange(len(index), device=logits.device).split(chunk):
        masks[part] = (upsample_host(logits[index[part]], input_size, mask_size, dtype, direct) > MASK_THRESHOLD).to(torch.uint8)
    return dict(masks=masks, index=index, area=area[index], boxes=boxes[index], predicted_iou=scores[index],
                stability_score=stab[index], keep_in=keep_in, stability_all=stab)


# ---------------------------------------------------------------- the generator
def grid_positional(G, g):
    """f32 [256,g,g]: get_image_wide_positional_embeddings in fp32 from the Gaussian matrix G f32 [2,128], on G's device (host_decoder's
    wide without the batch axis)."""
    c = (torch.arange(g, device=G.device, dtype=torch.float32) + 0.5) / g
    xy = 2 * torch.stack([c[None, :].expand(g, g), c[:, None].expand(g, g)], -1) - 1
    arg = 2 * np.pi * (xy @ G.to(torch.float32))
    return torch.cat([torch.sin(arg), torch.cos(arg)], -1).permute(2, 0, 1).contiguous()


def decode_chunk(workspace_bytes, g, P):
    """(points per call, bytes of workspace per call) for P points at grid g: as many points as DECODER_WORKSPACE_BUDGET, read
    now, holds (at least one, at most 65535); workspace_bytes(g, points) is the library's size function."""
    one = workspace_bytes(g, 1)
    per = max(1, workspace_bytes(g, 2) - one)
    chunk = int(min(P, 65535, max(1, 1 + (DECODER_WORKSPACE_BUDGET - one) // per)))
    while chunk > 1 and workspace_bytes(g, chunk) > DECODER_WORKSPACE_BUDGET:
        chunk -= 1
    return chunk, workspace_bytes(g, chunk)


class SamMaskGenerator:
    """The reference's SamAutomaticMaskGenerator for one full-image crop.  host=True: the encoder through transformers'
    SamVisionEncoder in fp32 and the selection through select_host, on the same device.
    Every step lives here once.  What a model supplies (sam2.Sam2MaskGenerator does, and overrides nothing else) are the class
    attributes below and the four methods marked "hook"."""
    WHO = "sam"
    ENCODER = SamImageEncoder                       # encode(pixel_values) on the kernels
    preprocess = staticmethod(preprocess)
    host_decoder = staticmethod(host_decoder)       # (weights, dtype, device) -> the torch modules and `wide`
    DIRECT = False                                  # the selection resamples in one step (SM_SCORE / SM_EMIT's *_direct entries)
    DECODE = ("gsr_sam_decode", "gsr_sam_decode_workspace_bytes")
    HOST_HIP = (ValueError, "cannot be combined with it")

    def __init__(self, weights, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.86, stability_score_thresh=0.92,
                 stability_score_offset=1.0, box_nms_thresh=0.7, host=False, device="cuda", decoder="torch"):
        if not weights.decoder:
            raise ValueError(f"{self.WHO}: the mask generator needs weights with the prompt encoder and the mask decoder")
        if decoder not in ("torch", "hip"):
            raise ValueError(f"{self.WHO}: decoder {decoder!r} is not 'torch' or 'hip'")
        if host and decoder == "hip":
            raise self.HOST_HIP[0](f"{self.WHO}: host=True runs the torch modules only; decoder='hip' {self.HOST_HIP[1]}")
        self.weights, self.config, self.device, self.host = weights, weights.config, torch.device(device), bool(host)
        self.decoder = decoder
        self.points_per_side, self.points_per_batch = int(points_per_side), int(points_per_batch)
        self.pred_iou_thresh, self.stability_score_thresh = float(pred_iou_thresh), float(stability_score_thresh)
        self.stability_score_offset, self.box_nms_thresh = float(stability_score_offset), float(box_nms_thresh)
        self.encoder = None if host else self.ENCODER(weights)
        self._host_model = self._modules = self._hip = None
        self.last_ms = {}

    # -- hook: the encoder's twin in fp32 on pixel_values [3,S,S], as encoder.encode returns it
    def _embed_host(self, x):
        if self._host_model is None:
            self._host_model = host_encoder(self.weights, torch.float32, self.device)
        return sam_host(self.weights, x, torch.float32, self.device, self._host_model)

    # -- hook: the torch decode call on what embed returned
    def _decode_torch(self, emb, points):
        return decode_host(self.weights, emb, self._decoder()[2], points, torch.float32, self.device, self._decoder(), self.points_per_batch)

    # -- hook: the embedding as the maps of the decode call, in its argument order
    def _maps(self, emb):
        g = self.config.grid
        return [emb.reshape(DECODER_CHANNELS, g, g)]

    # -- hook: what decoder="hip" is not built for
    def _check_hip(self):
        if self.config.grid > 64:
            raise NotImplementedError(f"sam: decoder='hip' is built for grids up to 64 (image_size <= 1024), not {self.config.grid}")

    # -- the torch modules of the decoder
    def _decoder(self):
        if self._modules is None:
            self._modules = self.host_decoder(self.weights, torch.float32, self.device)
        return self._modules

    # -- the weight table of the decode call and the positional embedding of the grid
    def _decoder_hip(self):
        if self._hip is None:
            self._check_hip()
            tensors = self.weights.copy(keep=lambda k: not k.startswith(VISION), device=self.device).decoder_table()
            table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            self._hip = dict(tensors=tensors, table=table, n=len(tensors), wide=grid_positional(tensors[0], self.config.image_size // PATCH))
        return self._hip

    @torch.no_grad()
    def embed(self, image):
        """HxWx3 uint8 -> dict(emb on the device, input_size, mask_size).  emb: f32 [1,C,g,g]; for SAM2 its three f32 maps."""
        x, input_size, mask_size = self.preprocess(image, self.config.image_size)
        x = x.to(self.device)
        emb = self._embed_host(x) if self.host else self.encoder.encode(x)
        emb = emb[None].to(torch.float32) if isinstance(emb, torch.Tensor) else [m.to(torch.float32) for m in emb]
        return dict(emb=emb, input_size=input_size, mask_size=mask_size)

    @torch.no_grad()
    def decode(self, emb, points):
        """emb as embed returns it, points f32 [P,2] (x, y) in the input frame -> (low_res f32 [P,3,L,L], iou f32 [P,3]).
        decoder="torch": transformers' modules in fp32, points_per_batch at a time; "hip": gsr_sam_decode (gsr_sam2_decode), as
        many points per call as sam.DECODER_WORKSPACE_BUDGET bytes of workspace hold."""
        if self.decoder == "hip":
            return self._decode_hip(emb, points)
        low, iou = self._decode_torch(emb, points)
        return low.to(torch.float32).contiguous(), iou.to(torch.float32).contiguous()

    def _decode_hip(self, emb, points):
        maps = self._maps(emb)
        if not all(m.is_cuda for m in maps):
            raise _lib.GsrError(f"{self.WHO}: decoder='hip' needs the embedding on the device (no CPU path; see decode_host / decode_host2)")
        d, L, S = self._decoder_hip(), _lib.lib(), self.config.image_size
        g, dev = S // PATCH, maps[-1].device
        maps = [m.to(torch.float32).contiguous() for m in maps]
        pts = points.to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
        P = pts.shape[0]
        low = torch.empty(P, 3, 4 * g, 4 * g, dtype=torch.float32, device=dev)
        iou = torch.empty(P, 3, dtype=torch.float32, device=dev)
        if P == 0:
            return low, iou
        decode, workspace_bytes = (getattr(L, name) for name in self.DECODE)
        chunk, nbytes = decode_chunk(workspace_bytes, g, P)
        ws = workspace(nbytes, dev)
        for k in range(0, P, chunk):
            n = min(chunk, P - k)
            _lib.check(decode(g, d["table"], d["n"], *[ptr(m) for m in maps], ptr(d["wide"]), ptr(pts[k:k + n]), n, S, ptr(ws), nbytes,
                              ptr(low[k:k + n]), ptr(iou[k:k + n]), stream(dev)))
        return low, iou

    @torch.no_grad()
    def select(self, low_res, iou, input_size, mask_size):
        """The reference's gates in its order: iou > pred_iou_thresh; inter / union >= stability_score_thresh (0 / 0 is
        rejected); SM_NMS; SM_EMIT.  Candidates are ordered point-major, then mask index.  One host synchronisation, for
        the kept count.  DIRECT (SAM2): the planes are resampled in ONE step from the L x L logits to mask_size (SAM2's
        postprocess_masks) and input_size is not read.
        -> dict(masks uint8 [m,oh,ow], index, area, boxes XYXY inclusive, predicted_iou, stability_score)."""
        args = (self.pred_iou_thresh, self.stability_score_thresh, self.stability_score_offset, self.box_nms_thresh)
        if self.host:
            return select_host(low_res, iou, input_size, mask_size, *args, direct=self.DIRECT)
        if not low_res.is_cuda:
            raise _lib.GsrError(f"{self.WHO}: select needs device tensors (no CPU path; see select_host)")
        dev, Lr = low_res.device, int(low_res.shape[-1])
        logits = low_res.reshape(-1, Lr, Lr).to(torch.float32).contiguous()
        scores = iou.reshape(-1).to(torch.float32).contiguous()
        n = logits.shape[0]
        oh, ow = mask_size
        L = _lib.lib()
        frame = (oh, ow) if self.DIRECT else (*input_size, oh, ow)
        score, emit = (getattr(L, name + ("_direct" if self.DIRECT else "")) for name in ("gsr_sam_mask_score", "gsr_sam_mask_emit"))
        first = scores > self.pred_iou_thresh
        skip = (~first).to(torch.uint8)
        counts = torch.empty(n, 3, dtype=torch.int32, device=dev)
        boxes = torch.empty(n, 4, dtype=torch.float32, device=dev)
        _lib.check(score(ptr(logits), n, Lr, *frame, MASK_THRESHOLD, self.stability_score_offset, ptr(skip), ptr(counts), ptr(boxes),
                         stream(dev)))
        stab = counts[:, 1].to(torch.float32) / counts[:, 2].to(torch.float32)
        keep_in = (first & (stab >= self.stability_score_thresh)).to(torch.uint8)
        kept = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        nbytes = L.gsr_sam_nms_workspace_bytes(n)
        ws = workspace(nbytes, dev)
        _lib.check(L.gsr_sam_nms(ptr(boxes), ptr(scores), ptr(keep_in), n, self.box_nms_thresh, ptr(ws), nbytes, ptr(kept), ptr(count),
                                 stream(dev)))
        m = int(count.item())           # the one synchronisation
        index = kept[:m].contiguous()
        masks = torch.empty(m, oh, ow, dtype=torch.uint8, device=dev)
        _lib.check(emit(ptr(logits), n, Lr, *frame, MASK_THRESHOLD, ptr(index), m, ptr(masks), stream(dev)))
        idx = index.to(torch.int64)
        return dict(masks=masks, index=idx, area=counts[idx, 0].to(torch.int64), boxes=boxes[idx], predicted_iou=scores[idx],
                    stability_score=stab[idx], keep_in=keep_in.to(torch.bool), stability_all=stab)

    def _run(self, image):
        def tick():
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            return time.perf_counter()
        t0 = tick()
        e = self.embed(image)
        t1 = tick()
        points = point_grid(self.points_per_side, e["input_size"])
        low, iou = self.decode(e["emb"], points)
        t2 = tick()
        sel = self.select(low, iou, e["input_size"], e["mask_size"])
        t3 = tick()
        self.last_ms = {"embed": 1e3 * (t1 - t0), "decode": 1e3 * (t2 - t1), "select": 1e3 * (t3 - t2)}
        return e, points, sel

    def generate_device(self, image):
        """uint8 [m,oh,ow] on the device, in NMS order: index k is segment id k in segment_init.label_points."""
        return self._run(image)[2]["masks"]

    def generate_segments(self, image):
        """(generate_device's masks, still on the device; what save_segments_boxes stores for generate's list: dict(masks bool
        [m,oh,ow], boxes XYXY = [x, y, x + w, y + h] i64 [m,4], areas i64 [m]) on the host) from ONE run and one copy of the masks:
        gaussmart_amd.identify_cli labels the cloud from the first and writes segments_NNN.npz from the second."""
        sel = self._run(image)[2]
        host = dict(masks=sel["masks"].cpu().numpy().astype(bool), boxes=sel["boxes"].cpu().numpy().astype(np.int64).reshape(-1, 4),
                    areas=sel["area"].cpu().numpy().astype(np.int64).reshape(-1))
        return sel["masks"], host

    def generate(self, image):
        """The reference's list of dicts, in NMS order."""
        e, points, sel = self._run(image)
        (ih, iw), (oh, ow) = e["input_size"], e["mask_size"]
        masks = sel["masks"].cpu().numpy().astype(bool)
        boxes, area = sel["boxes"].cpu().numpy(), sel["area"].cpu().numpy()
        piou, stab, index = sel["predicted_iou"].cpu().numpy(), sel["stability_score"].cpu().numpy(), sel["index"].cpu().numpy()
        pts = points.numpy().astype(np.float64) * np.array([ow / iw, oh / ih])
        out = []
        for k in range(len(index)):
            x0, y0, x1, y1 = (int(v) for v in boxes[k])
            out.append({"segmentation": masks[k], "area": int(area[k]), "bbox": [x0, y0, x1 - x0, y1 - y0],
                        "predicted_iou": float(piou[k]), "point_coords": [[float(v) for v in pts[index[k] // 3]]],
                        "stability_score": float(stab[k]), "crop_box": [0, 0, ow, oh]})
        return out


def save_segments_boxes(masks, path):
    """identification/sam.py:118-134: masks, boxes as XYXY = [x, y, x + w, y + h], areas."""
    seg = [m["segmentation"] for m in masks]
    boxes = [[m["bbox"][0], m["bbox"][1], m["bbox"][0] + m["bbox"][2], m["bbox"][1] + m["bbox"][3]] for m in masks]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, masks=np.array(seg), boxes=np.array(boxes), areas=np.array([m["area"] for m in masks]))
