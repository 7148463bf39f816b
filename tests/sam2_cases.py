"""Shared weights, inputs, twins and bars for tests/test_sam2_cpu.py and tests/test_gpu_sam2.py.

Weights: gaussmart_amd.sam2.random_sam2_weights' recipe (default initialisation zeroes both position tables and
no_memory_embedding).  256 FPN channels throughout: the stock mask decoder's conv_s0 / conv_s1 read that many.  pixel_values:
N(0, 1) rounded to fp16.  The weight seeds: the first bar condition (the fp16 twin's error below 1e-3 of a map's max-abs
value) is tight by construction for the third map, which the fp16 model rounds three times at values up to 16 (spacing 2^-7);
it comes out between 0.93e-3 and 1.26e-3 over seeds, and differs by up to 15 % between torch's two CPU paths for fp16
products (oneDNN, and the plain one where oneDNN has no fp16 kernels).  SEEDS are the best of 40 (H2) and of 13 (H1) tried:
0.93e-3 and 0.95e-3 at the worst over both paths.

The independent twin is transformers' own Sam2Model.get_image_embeddings on the CPU holding the same tensors
(gaussmart_amd.sam2.sam2_host), in fp64 (the truth), in fp16 (the library's own formulation: its error is the yardstick of the
whole-encoder bar, per output map), and in fp64 with one wrong reading each of the network (WRONG): every one of them must
move at least one map far beyond the bar."""
import functools

import torch
import torch.nn.functional as F

import sam_cases as SC1
from sam_cases import U16, U32, TINY16, round16
from gaussmart_amd import sam as S1
from gaussmart_amd import sam2 as S2

# name -> (embed, heads, blocks, global blocks); S = 256: the stage grids are 64 / 32 / 16 / 8, the stock windows 8 / 4 / 16 / 8
ENCODER_CASES = {"H1": (144, 2, (1, 2, 3, 2), (4,)),       # head_dim 72, widths 144 / 288 / 576 / 1152
                 "H2": (96, 1, (1, 1, 2, 1), (3,))}        # head_dim 96, K = 96
IMAGE = 256
SEEDS = {"H1": 2614, "H2": 127}
WRONG = ("no_window", "no_background", "no_top_down", "avg_pool", "all_global")


def config(name):
    embed, heads, blocks, glob = ENCODER_CASES[name]
    return S2.Sam2Config(embed_dim=embed, num_heads=heads, blocks_per_stage=blocks, global_attention_blocks=glob, image_size=IMAGE)


@functools.lru_cache(maxsize=None)
def weights(name):
    return S2.random_sam2_weights(config(name), seed=SEEDS[name])


@functools.lru_cache(maxsize=None)
def pixels(name):
    g = torch.Generator().manual_seed(ENCODER_CASES[name][0])
    return torch.randn(3, IMAGE, IMAGE, generator=g).to(torch.float16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def twin(name, dtype=torch.float64, variant="plain"):
    """The three maps of pixels(name) through transformers' Sam2Model in `dtype` on the CPU, as fp64 (once per session)."""
    from transformers.models.sam2 import modeling_sam2 as M
    w = weights(name)
    model = S2.host_model(w, dtype, "cpu")
    backbone = model.vision_encoder.backbone
    saved = M.do_pool
    with torch.no_grad():
        if variant == "no_window":
            backbone.pos_embed_window.zero_()
        elif variant == "no_background":
            backbone.pos_embed.zero_()
        elif variant == "no_top_down":
            model.vision_encoder.neck.fpn_top_down_levels = []
        elif variant == "all_global":
            for block in backbone.blocks:
                if not block.query_stride:
                    block.window_size = 0
        elif variant == "avg_pool":
            def avg(x, query_stride=None):
                return x if query_stride is None else F.avg_pool2d(x.permute(0, 3, 1, 2), query_stride, query_stride).permute(0, 2, 3, 1)
            M.do_pool = avg
        elif variant != "plain":
            raise ValueError(variant)
    try:
        return tuple(m.double() for m in S2.sam2_host(w, pixels(name), dtype, "cpu", model))
    finally:
        M.do_pool = saved


@functools.lru_cache(maxsize=None)
def model_bars(name):
    """Per output map: bar = 2 x the max-abs error of the twin in fp16 against the twin in fp64 on the same inputs (the factor
    2 as in sam_cases.model_bars: the two formulations round at different points and each is a single draw), and the map's
    max-abs value."""
    o64, o16 = twin(name), twin(name, torch.float16)
    out = []
    for k in range(3):
        e16 = float((o16[k] - o64[k]).abs().max())
        out.append({"bar": 2 * e16, "e16": e16, "max": float(o64[k].abs().max())})
    return out


@functools.lru_cache(maxsize=None)
def wrong_moves(name):
    """Per output map: how far every wrong reading of the network moves the fp64 twin (max-abs)."""
    o64 = twin(name)
    return [{v: float((twin(name, variant=v)[k] - o64[k]).abs().max()) for v in WRONG} for k in range(3)]


def check_bar_conditions(bars, moves):
    for b in bars:
        assert b["e16"] < 1e-3 * b["max"], b                                            # the yardstick itself is small
    for v in WRONG:
        assert any(m[v] > 10 * b["bar"] for b, m in zip(bars, moves)), (v, bars, moves)     # no wrong reading can hide in every map


def bars_line(name, bars, moves=None):
    return "\n".join(f"encoder {name} map {k}: max {b['max']:.3f}, twin fp16 error {b['e16']:.3e}, bar {b['bar']:.3e}"
                     + ("" if moves is None else "; moved by " + ", ".join(f"{v} {moves[k][v]:.3e}" for v in WRONG)) for k, b in enumerate(bars))


# ---------------------------------------------------------------- HV_ATTN in fp64
def attention64(qkv, g, w, stride, heads, hd):
    """fp64 (out [T_out,hidden], bar) of the HV_ATTN rule from fp16 inputs.  The bar follows the rule's stated roundings as
    sam_cases.attention64's does, with the two fp32 roundings of the score (the scale and the log2 e products, and the two
    constants' own rounding)."""
    s = g if w == 0 else w
    nw, sq, hidden = g // s, s // stride, heads * hd
    win = qkv.double().reshape(nw, s, nw, s, 3, heads, hd).permute(0, 2, 4, 5, 1, 3, 6).reshape(nw * nw, 3, heads, s, s, hd)
    q, k, v = win[:, 0], win[:, 1].reshape(nw * nw, heads, s * s, hd), win[:, 2].reshape(nw * nw, heads, s * s, hd)
    if stride == 2:
        q = q.reshape(nw * nw, heads, sq, 2, sq, 2, hd).amax((3, 5))
    q = q.reshape(nw * nw, heads, sq * sq, hd)
    scale = hd ** -0.5
    qk = q @ k.transpose(-1, -2)
    t = qk * scale
    p = torch.softmax(t, -1)
    o = p @ v
    chain = hd * U32 * ((q.abs() @ k.abs().transpose(-1, -2)) * scale)
    es = chain + 4 * U32 * t.abs()
    spread = (t.max(-1, keepdim=True).values - t).max(-1, keepdim=True).values
    delta = 2 * es.max(-1, keepdim=True).values + U32 * spread + 4 * U32
    A = p @ v.abs()
    e = (U16 + 2 * delta + (4 * s * s + 16) * U32) * A + TINY16 * v.abs().sum(-2, keepdim=True)
    bar = e + round16(o, e)

    def back(x):        # [W,heads,sq sq,hd] -> [T_out,hidden]
        return x.reshape(nw, nw, heads, sq, sq, hd).permute(0, 3, 1, 4, 2, 5).reshape(nw * sq * nw * sq, hidden)
    return back(o), back(bar)


# ---------------------------------------------------------------- the one-step mask route
# (L, the input size sam_cases.mask_logits centres its cones in, mask size, masks): the logits of tests/test_gpu_sam.py
MASK_SHAPES = [(40, (120, 160), (120, 160), 24), (40, (160, 120), (213, 160), 24), (40, (120, 160), (73, 97), 24),
               (64, (256, 171), (1000, 668), 200)]


def mask_truth(logits, mask_size, tau=0.0, delta=1.0, chunk=25, two_step=None):
    """sam_cases.mask_truth for SAM2's one F.interpolate from L x L to mask_size.  two_step: an input size; the planes of
    SAM's route (L -> 4 L, crop, resize) are judged instead, with the same decided set of the one-step values."""
    eps = 32 * U32 * float(logits.abs().max())
    on, decided, counts = [], [], []
    for part in logits.split(chunk):
        v = S1.upsample_host(part, None, mask_size, torch.float64, direct=True)
        decided.append(((v - (tau - delta)).abs() > eps) & ((v - tau).abs() > eps) & ((v - (tau + delta)).abs() > eps))
        if two_step is not None:
            v = S1.upsample_host(part, two_step, mask_size, torch.float64)
        on.append(v > tau)
        counts.append(torch.stack([(v > tau).flatten(1).sum(1), (v > tau + delta).flatten(1).sum(1), (v > tau - delta).flatten(1).sum(1)], 1))
    return {"on": torch.cat(on), "decided": torch.cat(decided), "counts": torch.cat(counts)}


def interpolate_loop(logits, mask_size):
    """One F.interpolate per mask, the plainest form of SAM2's postprocess_masks (in the logits' dtype)."""
    return torch.stack([F.interpolate(m[None, None], tuple(mask_size), mode="bilinear", align_corners=False)[0, 0] for m in logits])


mask_logits = SC1.mask_logits
