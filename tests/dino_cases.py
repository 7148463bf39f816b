"""Shared weights, images, twins and rounding bars for tests/test_dino_cpu.py and tests/test_gpu_dino.py.

Weights: default HF initialisation (std 0.02) is useless here -- the attention comes out uniform and RoPE, the biases and
LayerScale are invisible in the output -- so the recipe is gaussmart_amd.dino.random_dino_weights': linear and patch weights
N(0, 1/fan_in), LayerScale and LayerNorm gains U(0.5, 1.5), biases N(0, 0.1^2), CLS and register tokens N(0, 1), everything
rounded to fp16.  Images: image 0 is uniform noise in [0,1], image 1 is 0.5 image0 + 0.5 (y, x, xy ramps).

The independent twin is transformers' own DINOv3ViTModel on the CPU holding the same tensors (gaussmart_amd.dino.dino_host),
in fp64 (the truth), fp16 (the reference's formulation: its error is the yardstick of the whole-model bar) and fp64 with the
rotary embedding removed (the bar must be far below what a missing RoPE changes).
"""
import functools

import torch

from gaussmart_amd import dino as D

U16, U32 = 2.0 ** -11, 2.0 ** -24          # unit roundoffs of fp16 and fp32 (round to nearest)
TINY16 = 2.0 ** -25                        # half the spacing of fp16's subnormals

# name -> (hidden, heads, layers); intermediate = 4 hidden, 4 register tokens
CONFIGS = {"A": (128, 2, 2), "B": (128, 2, 3), "C": (768, 12, 1)}
# (config, H, W): T = 20 (less than any tile), 131 (one full 128-tile plus a 3-row tail), 277 (several tiles plus a tail)
MODEL_CASES = [("A", 48, 80), ("A", 144, 224), ("B", 272, 256), ("C", 144, 224)]


def config(name, registers=4):
    hidden, heads, layers = CONFIGS[name]
    return D.DinoConfig(hidden_size=hidden, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=4 * hidden,
                        num_register_tokens=registers)


@functools.lru_cache(maxsize=None)
def weights(name, registers=4):
    return D.random_dino_weights(config(name, registers), seed=1234 + registers)


@functools.lru_cache(maxsize=None)
def images(H, W):
    """float32 [2,3,H,W] on the CPU."""
    g = torch.Generator().manual_seed(1000 * H + W)
    a = torch.rand(3, H, W, generator=g)
    y = torch.linspace(0, 1, H)[:, None].expand(H, W)
    x = torch.linspace(0, 1, W)[None, :].expand(H, W)
    return torch.stack([a, 0.5 * a + 0.5 * torch.stack([y, x, y * x])])


def _no_rope(model):
    def forward(pixel_values):
        n = (pixel_values.shape[-2] // D.PATCH) * (pixel_values.shape[-1] // D.PATCH)
        return (torch.ones(n, D.HEAD_DIM, dtype=pixel_values.dtype), torch.zeros(n, D.HEAD_DIM, dtype=pixel_values.dtype))
    model.rope_embeddings.forward = forward
    return model


@functools.lru_cache(maxsize=None)
def twin(name, H, W, dtype=torch.float64, rope=True, registers=4):
    """(last_hidden [2,T,hidden], pooled [2,hidden]) of images(H, W) through the library's model in `dtype` on the CPU, as
    fp64 tensors (computed once per session)."""
    w = weights(name, registers)
    model = D.host_model(w, dtype, "cpu")
    if not rope:
        model = _no_rope(model)
    last, pooled = D.dino_host(w, images(H, W), dtype, "cpu", model)
    return last.double(), pooled.double()


@functools.lru_cache(maxsize=None)
def model_bars(name, H, W):
    """The whole-model rule.  bar = 2 x the max-abs error of the library's fp16 model against its fp64 model on the same
    inputs (the factor 2: the two formulations round at different points and each is a single draw), per output.  Returns
    {"last": bar, "pooled": bar, "e16": (last, pooled), "no_rope": (last, pooled) change when RoPE is removed, "cos": fp64
    cosine of the two images' pooled rows}; check_bar_conditions() holds what keeps the bar honest."""
    l64, p64 = twin(name, H, W, torch.float64)
    l16, p16 = twin(name, H, W, torch.float16)
    ln, pn = twin(name, H, W, torch.float64, rope=False)
    e = (float((l16 - l64).abs().max()), float((p16 - p64).abs().max()))
    cos = float(torch.nn.functional.cosine_similarity(p64[0], p64[1], dim=0))
    return {"last": 2 * e[0], "pooled": 2 * e[1], "e16": e, "no_rope": (float((ln - l64).abs().max()), float((pn - p64).abs().max())),
            "cos": cos}


def check_bar_conditions(bars):
    assert bars["e16"][0] < 1e-2 and bars["e16"][1] < 1e-2, bars          # the yardstick itself is small
    assert bars["no_rope"][0] > 10 * bars["last"] and bars["no_rope"][1] > 10 * bars["pooled"], bars   # a missing RoPE cannot hide
    assert bars["cos"] < 0.97, bars                                       # the two images are told apart


# ---------------------------------------------------------------- per-stage bars, from include/gsr.h's stated roundings
def round16(v, e=0.0):
    """Bound of one rounding to fp16 of a value within e of v."""
    return U16 * (v.abs() + e) + TINY16


def linear_bars(x, w, b, lam=None, resid=None):
    """x fp16 [M,K], w fp16 [N,K], b fp16 [N] or None -> fp64 (u, S, E): u = x w^T + b, S = sum_k |x_k w_k|, and the fp32 error
    E of the accumulated value plus bias: K 2^-24 S for the chain (each of the K additions rounds a partial sum below S)
    and 2^-24 |u| for the bias addition."""
    x64, w64 = x.double().cpu(), w.double().cpu()
    u = x64 @ w64.T + (b.double().cpu() if b is not None else 0.0)
    S = x64.abs() @ w64.abs().T
    return u, S, x.shape[1] * U32 * S + U32 * u.abs()


def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / 2.0 ** 0.5))
