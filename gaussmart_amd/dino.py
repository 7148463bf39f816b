"""DINOv3 ViT image encoder on the device: the reference's DINOImageEncoder (identification/feature_extraction.py:18-43, a
transformers DINOv3ViTModel in fp16) computed by the kernels of csrc/dino.hip and csrc/vit.hip (include/gsr.h: DN_EMBED, DN_NORM, DN_LINEAR,
DN_ROPE, DN_ATTN, DN_POOL, DN_COS).

    from gaussmart_amd.dino import DINOImageEncoder, load_dino_weights
    enc = DINOImageEncoder("/models/dinov3-vitb16")            # a LOCAL directory, see below
    emb = enc.encode_tensor(image)                              # [hidden], the pooled (CLS) row, as the reference returns it
    both = enc.encode_pair(render, gt)                          # [2,hidden], one pass over both images
    tokens = enc.encode_tokens(image)                           # [T,hidden], last_hidden_state

What differs from the reference, on purpose:
  * nothing is fetched and no hub login happens: `load_dino_weights` takes a directory holding config.json,
    preprocessor_config.json and model.safetensors (or pytorch_model.bin), i.e. what `save_pretrained` writes; a hub name is
    refused.
  * the weights are fp16 as the reference's .half() makes them, but the residual stream, the LayerNorm statistics and the
    softmax are fp32 (the reference keeps everything in fp16), and the embedding comes back as fp32.
  * CPU tensors are refused: `dino_host` is the transformers formulation from the same tensors (any dtype, any device),
    which serves train_cli --host and the tests.
Inference only: no gradient flows through the encoder (the reference runs it under inference_mode as well).
"""
import ctypes as C
import json
import math
import os
from dataclasses import dataclass, field, asdict

import torch

from . import _lib
from ._dev import ptr, stream, workspace

PATCH = 16
HEAD_DIM = 64
# per layer, in the order of include/gsr.h's GSR_DINO_L_*: state-dict name under "<layer prefix>.<l>.", and whether it may be absent
LAYER_KEYS = (("norm1.weight", False), ("norm1.bias", False),
              ("attention.q_proj.weight", False), ("attention.q_proj.bias", True),
              ("attention.k_proj.weight", False), ("attention.k_proj.bias", True),
              ("attention.v_proj.weight", False), ("attention.v_proj.bias", True),
              ("attention.o_proj.weight", False), ("attention.o_proj.bias", True),
              ("layer_scale1.lambda1", False), ("norm2.weight", False), ("norm2.bias", False),
              ("mlp.up_proj.weight", False), ("mlp.up_proj.bias", True),
              ("mlp.down_proj.weight", False), ("mlp.down_proj.bias", True), ("layer_scale2.lambda1", False))
HEAD_KEYS = ("embeddings.cls_token", "embeddings.register_tokens", "embeddings.patch_embeddings.weight",
             "embeddings.patch_embeddings.bias")
TAIL_KEYS = ("norm.weight", "norm.bias")
assert len(LAYER_KEYS) == _lib.GSR_DINO_W_PER_LAYER and len(HEAD_KEYS) == _lib.GSR_DINO_W_LAYER0


def _layer_prefix():
    """"model.layer" or "layer": whatever the installed transformers' DINOv3ViTModel.state_dict() uses."""
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    cfg = DINOv3ViTConfig(hidden_size=64, num_attention_heads=1, num_hidden_layers=1, intermediate_size=64)
    with torch.device("meta"):
        keys = DINOv3ViTModel(cfg).state_dict().keys()
    return "model.layer" if any(k.startswith("model.layer.") for k in keys) else "layer"


@dataclass
class DinoConfig:
    """Defaults: facebook/dinov3-vitb16 (ViT-B/16, 4 register tokens, no key bias, ungated GELU, ImageNet statistics)."""
    hidden_size: int = 768
    num_attention_heads: int = 12
    num_hidden_layers: int = 12
    intermediate_size: int = 3072
    num_register_tokens: int = 4
    rope_theta: float = 100.0
    layer_norm_eps: float = 1e-5
    query_bias: bool = True
    key_bias: bool = False
    value_bias: bool = True
    proj_bias: bool = True
    mlp_bias: bool = True
    hidden_act: str = "gelu"
    use_gated_mlp: bool = False
    patch_size: int = PATCH
    image_mean: tuple = (0.485, 0.456, 0.406)
    image_std: tuple = (0.229, 0.224, 0.225)

    def check(self):
        if self.patch_size != PATCH:
            raise NotImplementedError(f"dino: patch size {self.patch_size} is not built (16 only)")
        if self.use_gated_mlp or self.hidden_act != "gelu":
            raise NotImplementedError("dino: only the ungated exact-GELU MLP is built")
        if self.hidden_size != HEAD_DIM * self.num_attention_heads:
            raise NotImplementedError(f"dino: hidden {self.hidden_size} is not 64 * heads ({self.num_attention_heads}); the head "
                                      "dimension is fixed at 64")
        return self

    def tokens(self, H, W):
        return 1 + self.num_register_tokens + (H // PATCH) * (W // PATCH)

    def has_bias(self, layer_key):
        return {"attention.q_proj.bias": self.query_bias, "attention.k_proj.bias": self.key_bias,
                "attention.v_proj.bias": self.value_bias, "attention.o_proj.bias": self.proj_bias,
                "mlp.up_proj.bias": self.mlp_bias, "mlp.down_proj.bias": self.mlp_bias}.get(layer_key, True)

    def to_hf(self):
        from transformers import DINOv3ViTConfig
        return DINOv3ViTConfig(hidden_size=self.hidden_size, num_attention_heads=self.num_attention_heads,
                               num_hidden_layers=self.num_hidden_layers, intermediate_size=self.intermediate_size,
                               num_register_tokens=self.num_register_tokens, rope_theta=self.rope_theta,
                               layer_norm_eps=self.layer_norm_eps, query_bias=self.query_bias, key_bias=self.key_bias,
                               value_bias=self.value_bias, proj_bias=self.proj_bias, mlp_bias=self.mlp_bias,
                               hidden_act=self.hidden_act, use_gated_mlp=self.use_gated_mlp, patch_size=self.patch_size)

    def to_c(self):
        self.check()
        c = _lib.GsrDinoConfig(self.hidden_size, self.num_attention_heads, self.num_hidden_layers, self.intermediate_size,
                               self.num_register_tokens, self.rope_theta, self.layer_norm_eps)
        c.image_mean[:] = [float(v) for v in self.image_mean]
        c.image_std[:] = [float(v) for v in self.image_std]
        return c


class DinoWeights:
    """config + the tensors under DINOv3ViTModel.state_dict()'s names (mask_token is not needed), rounded to fp16."""

    def __init__(self, config, tensors):
        self.config = config.check()
        self.prefix = _layer_prefix()
        self.tensors = {}
        for name in self.names():
            if name not in tensors:
                raise KeyError(f"dino weights: no tensor {name}")
            self.tensors[name] = tensors[name].detach().to(torch.float16).contiguous()
        c = config
        want = {"embeddings.cls_token": (1, 1, c.hidden_size),
                "embeddings.register_tokens": (1, c.num_register_tokens, c.hidden_size),
                "embeddings.patch_embeddings.weight": (c.hidden_size, 3, PATCH, PATCH),
                f"{self.prefix}.0.mlp.up_proj.weight": (c.intermediate_size, c.hidden_size)}
        for name, shape in want.items():
            if tuple(self.tensors[name].shape) != shape:
                raise ValueError(f"dino weights: {name} must be {list(shape)}, got {list(self.tensors[name].shape)}")

    def names(self):
        out = list(HEAD_KEYS)
        for l in range(self.config.num_hidden_layers):
            out += [f"{self.prefix}.{l}.{k}" for k, _ in LAYER_KEYS if self.config.has_bias(k)]
        return out + list(TAIL_KEYS)

    def to(self, device):
        w = DinoWeights.__new__(DinoWeights)
        w.config, w.prefix = self.config, self.prefix
        w.tensors = {k: t.to(device) for k, t in self.tensors.items()}
        return w

    def table(self):
        """The tensors in the order of gsr_dino_forward's weight table (None: an absent bias, or no registers)."""
        out = [self.tensors[k] for k in HEAD_KEYS]
        for l in range(self.config.num_hidden_layers):
            out += [self.tensors.get(f"{self.prefix}.{l}.{k}") for k, _ in LAYER_KEYS]
        return out + [self.tensors[k] for k in TAIL_KEYS]


def load_dino_weights(directory):
    """Reads config.json, preprocessor_config.json and model.safetensors / pytorch_model.bin of a LOCAL directory.  Nothing
    here opens a URL: a hub name ("facebook/dinov3-...") is not a directory and is refused."""
    directory = os.fspath(directory)
    if not os.path.isdir(directory):
        raise FileNotFoundError(f"dino: {directory!r} is not a local directory.  The weights are never downloaded: pass the "
                                "directory that holds config.json, preprocessor_config.json and model.safetensors")
    paths = {n: os.path.join(directory, n) for n in ("config.json", "preprocessor_config.json", "model.safetensors", "pytorch_model.bin")}
    for n in ("config.json", "preprocessor_config.json"):
        if not os.path.isfile(paths[n]):
            raise FileNotFoundError(f"dino: {paths[n]} not found")
    with open(paths["config.json"]) as f:
        hf = json.load(f)
    with open(paths["preprocessor_config.json"]) as f:
        pre = json.load(f)
    known = {f.name for f in DinoConfig.__dataclass_fields__.values()}
    cfg = DinoConfig(**{k: v for k, v in hf.items() if k in known and k not in ("image_mean", "image_std")})
    cfg.image_mean = tuple(pre.get("image_mean", cfg.image_mean))
    cfg.image_std = tuple(pre.get("image_std", cfg.image_std))
    if os.path.isfile(paths["model.safetensors"]):
        from safetensors.torch import load_file
        tensors = load_file(paths["model.safetensors"], device="cpu")
    elif os.path.isfile(paths["pytorch_model.bin"]):
        tensors = torch.load(paths["pytorch_model.bin"], map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"dino: neither {paths['model.safetensors']} nor {paths['pytorch_model.bin']} found")
    prefix = _layer_prefix()
    other = "layer" if prefix == "model.layer" else "model.layer"       # a file written by the other key layout
    tensors = {(prefix + k[len(other):] if k.startswith(other + ".") else k): v for k, v in tensors.items()}
    return DinoWeights(cfg, tensors)


def save_dino_weights(weights, directory):
    """Writes what load_dino_weights reads (config.json, preprocessor_config.json, model.safetensors)."""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    cfg = asdict(weights.config)
    pre = {"image_mean": list(cfg.pop("image_mean")), "image_std": list(cfg.pop("image_std"))}
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(dict(cfg, model_type="dinov3_vit"), f, indent=1)
    with open(os.path.join(directory, "preprocessor_config.json"), "w") as f:
        json.dump(pre, f, indent=1)
    tensors = {k: t.cpu().contiguous() for k, t in weights.tensors.items()}
    tensors["embeddings.mask_token"] = torch.zeros(1, 1, weights.config.hidden_size, dtype=torch.float16)
    save_file(tensors, os.path.join(directory, "model.safetensors"))


def random_dino_weights(config=None, seed=0):
    """Seeded stand-ins at a scale where every part of the network is visible in the output (what the benchmark and the
    tests run on): linear and patch weights N(0, 1/fan_in), LayerScale and LayerNorm gains U(0.5, 1.5), biases N(0, 0.1^2),
    CLS and register tokens N(0, 1); all rounded to fp16."""
    cfg = (config or DinoConfig()).check()
    g = torch.Generator().manual_seed(seed)
    w = DinoWeights.__new__(DinoWeights)
    w.config, w.prefix, w.tensors = cfg, _layer_prefix(), {}
    shapes = {"embeddings.cls_token": (1, 1, cfg.hidden_size), "embeddings.register_tokens": (1, cfg.num_register_tokens, cfg.hidden_size),
              "embeddings.patch_embeddings.weight": (cfg.hidden_size, 3, PATCH, PATCH), "embeddings.patch_embeddings.bias": (cfg.hidden_size,),
              "norm.weight": (cfg.hidden_size,), "norm.bias": (cfg.hidden_size,)}
    h, m = cfg.hidden_size, cfg.intermediate_size
    per_layer = {"norm1.weight": (h,), "norm1.bias": (h,), "norm2.weight": (h,), "norm2.bias": (h,), "layer_scale1.lambda1": (h,),
                 "layer_scale2.lambda1": (h,), "mlp.up_proj.weight": (m, h), "mlp.up_proj.bias": (m,), "mlp.down_proj.weight": (h, m),
                 "mlp.down_proj.bias": (h,)}
    for p in "qkvo":
        per_layer[f"attention.{p}_proj.weight"] = (h, h)
        per_layer[f"attention.{p}_proj.bias"] = (h,)
    for name in w.names():
        key = name.split(".", 2 + w.prefix.count("."))[-1] if name.startswith(w.prefix + ".") else name
        shape = shapes.get(name) or per_layer[key]
        if key.endswith("lambda1") or key in ("norm1.weight", "norm2.weight", "norm.weight"):
            t = 0.5 + torch.rand(shape, generator=g)
        elif key.endswith("_token") or key.endswith("register_tokens"):
            t = torch.randn(shape, generator=g)
        elif key.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = math.prod(shape[1:])
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        w.tensors[name] = t.to(torch.float16)
    return w


# ---------------------------------------------------------------- RoPE of the installed library's definition (host, any dtype)
def patch_coordinates(Hp, Wp, dtype=torch.float64):
    """[Hp Wp, 2]: (y, x) centres of the patches in [-1, 1] (get_patches_center_coordinates)."""
    ys = 2.0 * ((torch.arange(Hp, dtype=dtype) + 0.5) / Hp) - 1.0
    xs = 2.0 * ((torch.arange(Wp, dtype=dtype) + 0.5) / Wp) - 1.0
    return torch.stack(torch.meshgrid(ys, xs, indexing="ij"), dim=-1).flatten(0, 1)


def rope_table(Hp, Wp, theta=100.0, dtype=torch.float64):
    """(cos, sin), each [Hp Wp, 64]: angle = 2 pi coord theta^(-j / 16), laid out [y: 16, x: 16] and tiled twice."""
    inv_freq = 1.0 / torch.tensor(theta, dtype=dtype) ** (torch.arange(16, dtype=dtype) / 16.0)
    angles = 2.0 * math.pi * patch_coordinates(Hp, Wp, dtype)[:, :, None] * inv_freq[None, None, :]
    angles = angles.flatten(1, 2).tile(2)
    return torch.cos(angles), torch.sin(angles)


# ---------------------------------------------------------------- the twin
def host_model(weights, dtype=torch.float64, device="cpu"):
    """transformers' DINOv3ViTModel holding these tensors, in `dtype` on `device`, in eval mode."""
    from transformers import DINOv3ViTModel
    model = DINOv3ViTModel(weights.config.to_hf())
    sd = {k: t.to(torch.float32) for k, t in weights.tensors.items()}
    sd["embeddings.mask_token"] = torch.zeros(1, 1, weights.config.hidden_size)
    model.load_state_dict(sd, strict=True)
    return model.to(device=device, dtype=dtype).eval()


@torch.no_grad()
def dino_host(weights, images, dtype=torch.float64, device=None, model=None):
    """(last_hidden_state [B,T,hidden], pooler_output [B,hidden]) of images [B,3,H,W] (or [3,H,W]) through the library's own
    model: normalisation (x - mean) / std in `dtype`, as the reference's encode_tensor does it in fp16."""
    if images.dim() == 3:
        images = images[None]
    device = images.device if device is None else device
    model = host_model(weights, dtype, device) if model is None else model
    x = images.to(device=device, dtype=dtype)
    mean = torch.tensor(weights.config.image_mean, device=device, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(weights.config.image_std, device=device, dtype=dtype).view(1, 3, 1, 1)
    out = model((x - mean) / std)
    return out.last_hidden_state, out.pooler_output


# ---------------------------------------------------------------- the encoder
class DINOImageEncoder:
    """encode_tensor(image [3,H,W]) -> [hidden] as the reference's class, on the kernels; the result is fp32."""

    def __init__(self, weights_or_dir):
        self.weights = weights_or_dir if isinstance(weights_or_dir, DinoWeights) else load_dino_weights(weights_or_dir)
        self.config = self.weights.config
        self._on = {}           # device -> (weights there, host table of device pointers, GsrDinoConfig)
        self._ws = {}           # (device, B, H, W) -> workspace, kept: an encoder serves one image size over and over

    def _device(self, dev):
        hit = self._on.get(dev)
        if hit is None:
            w = self.weights.to(dev)
            tensors = w.table()
            table = (C.c_void_p * len(tensors))(*[t.data_ptr() if t is not None and t.numel() else None for t in tensors])
            hit = self._on[dev] = (w, table, len(tensors), self.config.to_c())
        return hit

    def _images(self, images):
        out = []
        for t in images:
            if not isinstance(t, torch.Tensor):
                raise TypeError("dino: images must be tensors")
            if t.dim() == 4 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 3 or t.shape[0] != 3:
                raise ValueError(f"dino: expected [3,H,W], got {list(t.shape)}")
            if not t.is_cuda:
                raise _lib.GsrError("dino: tensors must live on the device (no CPU path; see dino_host)")
            out.append(t.detach().to(torch.float32).contiguous())
        if any(t.shape != out[0].shape or t.device != out[0].device for t in out):
            raise ValueError("dino: the images of one call must have one shape and one device")
        return out

    @torch.no_grad()
    def forward(self, images, tokens=False):
        """images: a list of 1 or 2 tensors [3,H,W] (need not be contiguous with each other), or one tensor [B,3,H,W] with
        B <= 8.  -> (pooled [B,hidden], last_hidden [B,T,hidden] or None), fp32."""
        if isinstance(images, torch.Tensor) and images.dim() == 4:
            if not images.is_cuda:
                raise _lib.GsrError("dino: tensors must live on the device (no CPU path; see dino_host)")
            x = images.detach().to(torch.float32).contiguous()
            B, x0, x1, keep = x.shape[0], x, None, (x,)
            H, W = int(x.shape[2]), int(x.shape[3])
        else:
            keep = self._images(list(images))
            if len(keep) not in (1, 2):
                raise ValueError("dino: pass one or two separate images, or one [B,3,H,W] tensor")
            B, x0, x1 = len(keep), keep[0], keep[1] if len(keep) == 2 else None
            H, W = int(x0.shape[1]), int(x0.shape[2])
        dev = x0.device
        L = _lib.lib()
        _, table, n, cfg = self._device(dev)
        nbytes = L.gsr_dino_workspace_bytes(C.byref(cfg), B, H, W)
        if nbytes == 0:
            _lib.check(L.gsr_dino_forward(C.byref(cfg), table, n, ptr(x0), ptr(x1), B, H, W, None, 0, None, None, stream(dev)))
        ws = self._ws.get((dev, B, H, W))
        if ws is None:
            ws = self._ws[(dev, B, H, W)] = workspace(nbytes, dev)
        pooled = torch.empty(B, self.config.hidden_size, dtype=torch.float32, device=dev)
        last = torch.empty(B, self.config.tokens(H, W), self.config.hidden_size, dtype=torch.float32, device=dev) if tokens else None
        _lib.check(L.gsr_dino_forward(C.byref(cfg), table, n, ptr(x0), ptr(x1), B, H, W, ptr(ws), nbytes, ptr(pooled), ptr(last),
                                      stream(dev)))
        return pooled, last

    def encode_tensor(self, image_tensor):
        return self.forward([image_tensor])[0][0]

    def encode_pair(self, a, b):
        return self.forward([a, b])[0]

    def encode_tokens(self, image_tensor):
        return self.forward([image_tensor], tokens=True)[1][0]


class HostDINOImageEncoder:
    """The same interface on dino_host (transformers' model; fp32 by default, on the images' device): train_cli --host."""

    def __init__(self, weights_or_dir, dtype=torch.float32):
        self.weights = weights_or_dir if isinstance(weights_or_dir, DinoWeights) else load_dino_weights(weights_or_dir)
        self.config, self.dtype, self._models = self.weights.config, dtype, {}

    def _run(self, images):
        dev = images.device
        if dev not in self._models:
            self._models[dev] = host_model(self.weights, self.dtype, dev)
        return dino_host(self.weights, images, self.dtype, dev, self._models[dev])

    def encode_tensor(self, image_tensor):
        return self._run(image_tensor.detach())[1][0].float()

    def encode_pair(self, a, b):
        return self._run(torch.stack([a.detach(), b.detach()]))[1].float()

    def encode_tokens(self, image_tensor):
        return self._run(image_tensor.detach())[0][0].float()


def lambda_fp16(lambda_dino):
    """The reference multiplies by torch.tensor(lambda_dino, dtype=float16): that rounded value, as a float."""
    return float(torch.tensor(float(lambda_dino), dtype=torch.float16))


def scaled_cosine(a, b, lambda_dino):
    """fp32 0-dim: fp16(lambda) * cos(a, b), F.cosine_similarity's definition (eps 1e-8); device tensors through
    gsr_dino_cosine (DN_COS), host tensors through the same formula in torch."""
    lam = lambda_fp16(lambda_dino)
    a, b = a.detach().reshape(-1).to(torch.float32), b.detach().reshape(-1).to(torch.float32)
    if a.numel() != b.numel():
        raise ValueError(f"dino cosine: {a.numel()} vs {b.numel()} elements")
    if a.is_cuda:
        a, b = a.contiguous(), b.to(a.device).contiguous()
        out = torch.empty((), dtype=torch.float32, device=a.device)
        _lib.check(_lib.lib().gsr_dino_cosine(ptr(a), ptr(b), a.numel(), lam, ptr(out), stream(a.device)))
        return out
    na, nb = a.norm().clamp_min(1e-8), b.norm().clamp_min(1e-8)
    return lam * ((a * b).sum() / (na * nb))
