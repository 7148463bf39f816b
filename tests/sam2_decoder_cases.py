"""Shared cases, twins, fp64 restatements and bars for tests/test_sam2_decoder_cpu.py and tests/test_gpu_sam2_decoder.py.

Whole decoder: K1 (a one-block-per-stage Hiera at 128 x 128: g = 8, T = 64, 9 points) and K2 (sam2_cases' H2 configuration at
256 x 256: g = 16, T = 256, 67 points: more than 64 points and a tail).  The three maps are N(0,1) from generator seed 5, drawn
in the order [32,4g,4g], [64,2g,2g], [256,g,g] and rounded to fp16.  Truth is gaussmart_amd.sam2.decode_host2 in fp64 on the
CPU, the yardstick e16 the same modules in fp16 on the CPU, taken separately for the masks and for the IoU; bar = 2 x e16 (the
two formulations round at different points and each is a single draw).  The wrong readings (no image positional embedding,
no_mask_embed / feat_s0 / feat_s1 / obj_score_token zeroed, SAM's seven tokens without the object-score token) must move the
fp64 masks by more than 10 x bar, and so must neighbouring points.

Stages: fp64 restatements of SD_T2I, SD_I2T and SD_UP (include/gsr.h) with the S2D_* deltas (eight tokens, eps as an argument,
the two skips) from the same fp16-rounded inputs, with bars built from the roundings the rules state, as
tests/sam_decoder_cases.py builds them for SAM."""
import functools

import torch

import sam_decoder_cases as DC
from sam_cases import U32, round16
from gaussmart_amd import sam as S1
from gaussmart_amd import sam2 as S2

K1 = S2.Sam2Config(embed_dim=96, num_heads=1, blocks_per_stage=(1, 1, 1, 1), global_attention_blocks=(), window_size_per_stage=(8, 4, 4, 2),
                   image_size=128)
K2 = S2.Sam2Config(embed_dim=96, num_heads=1, blocks_per_stage=(1, 1, 2, 1), global_attention_blocks=(3,), image_size=256)
# name -> (configuration, weight seed, points per side of the grid, how many of its points)
DECODER_CASES = {"K1": (K1, 11, 3, 9), "K2": (K2, 127, 9, 67)}
VARIANTS = ("no_pe", "no_mask_embed", "no_feat_s0", "no_feat_s1", "seven_tokens", "no_obj_token")
MOVES_IOU = ("no_pe", "seven_tokens")           # these move the IoU by more than 10 x its bar too
tiny_scan, h16 = DC.tiny_scan, DC.h16


@functools.lru_cache(maxsize=None)
def weights(name):
    cfg, seed = DECODER_CASES[name][:2]
    return S2.random_sam2_weights(cfg, seed=seed)


@functools.lru_cache(maxsize=None)
def maps(name):
    g = weights(name).config.image_size // 16
    gen = torch.Generator().manual_seed(5)
    return tuple(torch.randn(shape, generator=gen).to(torch.float16).to(torch.float32) for shape in ((32, 4 * g, 4 * g), (64, 2 * g, 2 * g), (256, g, g)))


@functools.lru_cache(maxsize=None)
def points(name):
    cfg, _, side, n = DECODER_CASES[name]
    return S1.point_grid(side, (cfg.image_size, cfg.image_size))[:n].contiguous()


_without = DC._without


@torch.no_grad()
def modules_direct(modules, maps_, pts, dtype, obj_token=True):
    """Sam2PromptEncoder and the parts of Sam2MaskDecoder called one by one, all points in one batch -> (low_res [P,3,4g,4g],
    iou [P,3]).  obj_token=False is the wrong reading "SAM's seven tokens": no object-score token, the IoU token in row 0."""
    prompt, dec, wide = modules
    s0, s1, top = (m[None].to(dtype) for m in maps_)
    P = len(pts)
    sparse, dense = prompt(pts.to(dtype)[None, :, None, :], torch.ones(1, P, 1, dtype=torch.int64), None, None)
    rows = ([dec.obj_score_token.weight] if obj_token else []) + [dec.iou_token.weight, dec.mask_tokens.weight]
    o = int(obj_token)
    tokens = torch.cat((torch.cat(rows, 0).repeat(1, P, 1, 1), sparse.to(dtype)), 2)
    img = (top + dense).repeat_interleave(P, 0)
    tok, img = dec.transformer(point_embeddings=tokens, image_embeddings=img, image_positional_embeddings=wide.repeat_interleave(P, 0),
                               attention_similarity=None, target_embedding=None)
    g = top.shape[-1]
    img = img.transpose(2, 3).reshape(P, 256, g, g)
    up = dec.activation(dec.upscale_layer_norm(dec.upscale_conv1(img) + s1))
    up = dec.activation(dec.upscale_conv2(up) + s0)
    hyper = torch.stack([dec.output_hypernetworks_mlps[i](tok[:, :, o + 1 + i]) for i in range(4)], 2)          # [1,P,4,32]
    masks = (hyper[0] @ up.reshape(P, 32, -1)).reshape(P, 4, 4 * g, 4 * g)
    iou = dec.iou_prediction_head(tok[:, :, o])[0]
    return masks[:, 1:].contiguous(), iou[:, 1:].contiguous()


@functools.lru_cache(maxsize=None)
def twin(name, dtype=torch.float64, variant="plain"):
    """(low_res [P,3,4g,4g], iou [P,3]) as fp64, of decode_host2 in `dtype` on the CPU (computed once per session)."""
    w, m, pts = weights(name), list(maps(name)), points(name)
    if variant == "no_mask_embed":
        w = _without(w, "prompt_encoder.no_mask_embed.weight")
    elif variant == "no_obj_token":
        w = _without(w, S2.OBJ_TOKEN)
    elif variant == "no_feat_s0":
        m[0] = torch.zeros_like(m[0])
    elif variant == "no_feat_s1":
        m[1] = torch.zeros_like(m[1])
    modules = S2.host_decoder2(w, dtype, "cpu")
    if variant == "no_pe":
        modules = (modules[0], modules[1], torch.zeros_like(modules[2]))
    if variant == "seven_tokens":
        low, iou = modules_direct(modules, m, pts, dtype, obj_token=False)
    else:
        low, iou = S2.decode_host2(w, m, pts, dtype, "cpu", modules)
    return low.double(), iou.double()


@functools.lru_cache(maxsize=None)
def model_bars(name):
    low64, iou64 = twin(name)
    low16, iou16 = twin(name, torch.float16)
    e_mask, e_iou = float((low16 - low64).abs().max()), float((iou16 - iou64).abs().max())
    out = {"e16_mask": e_mask, "e16_iou": e_iou, "bar_mask": 2 * e_mask, "bar_iou": 2 * e_iou}
    for variant in VARIANTS:
        lo, io = twin(name, variant=variant)
        out[variant + "_mask"], out[variant + "_iou"] = float((lo - low64).abs().max()), float((io - iou64).abs().max())
    out["neighbours"] = float((low64[1:] - low64[:-1]).flatten(1).abs().max(1).values.min())
    return out


def check_bar_conditions(b):
    assert b["e16_mask"] < 3e-2 and b["e16_iou"] < 1e-2, b              # the yardsticks themselves are small
    for variant in VARIANTS:
        assert b[variant + "_mask"] > 10 * b["bar_mask"], (variant, b)
    for variant in MOVES_IOU:
        assert b[variant + "_iou"] > 10 * b["bar_iou"], (variant, b)
    assert b["neighbours"] > 10 * b["bar_mask"], b                      # points that got mixed up must show


def bars_line(name, b):
    moves = ", ".join(f"{v} {b[v + '_mask'] / b['bar_mask']:.0f}x" + (f" / {b[v + '_iou'] / b['bar_iou']:.0f}x" if v in MOVES_IOU else "")
                      for v in VARIANTS)
    return (f"decoder {name}: twin fp16 error masks {b['e16_mask']:.3e} iou {b['e16_iou']:.3e}, bars {b['bar_mask']:.3e} / {b['bar_iou']:.3e}; "
            f"moved by {moves}, neighbours {b['neighbours'] / b['bar_mask']:.0f}x")


# ---------------------------------------------------------------- fp64 restatements of the stage rules: SAM's, for eight tokens
t2i64 = DC.t2i64
i2t64 = functools.partial(DC.i2t64, eps=1e-5)       # layer_norm4's eps in SAM2; a call's own eps= still decides


def up64(x, g, c1w, c1b, lw, lb, c2w, c2b, hyper, s0, s1, s1_after_norm=False, s0_after_gelu=False, swap0=False, swap1=False):
    """SD_UP with S2D_UP's skips in fp64 from the module's own tensors -> (low_res [P,m,4g,4g], bar).  x fp16 [P,T,256]; c1w
    [256,64,2,2], c2w [64,32,2,2] as ConvTranspose2d holds them; hyper f32 [P,m,32]; s0 f32 [32,4g,4g], s1 f32 [64,2g,2g].  The
    wrong readings: s1 added after the LayerNorm, s0 added after the GELU, the (dy, dx) taps of a skip transposed."""
    P = x.shape[0]
    X = x.double().reshape(P, g, g, 256)
    W1, W2 = c1w.double(), c2w.double()
    # [64,2g,2g] -> [g,g,2,2,64] and [32,4g,4g] -> [g,g,2,2,2,2,32]: (y, x, dy, dx[, dy2, dx2], c)
    S1_ = s1.double().reshape(64, g, 2, g, 2).permute(1, 3, 2, 4, 0)
    S0_ = s0.double().reshape(32, g, 2, 2, g, 2, 2).permute(1, 4, 2, 5, 3, 6, 0)
    if swap1:
        S1_ = S1_.transpose(2, 3)
    if swap0:
        S0_ = S0_.transpose(2, 3).transpose(4, 5)
    u = torch.einsum("pyxi,iodk->pyxdko", X, W1) + c1b.double()                 # [P,g,g,2,2,64]
    e_u = (256 + 2) * U32 * (torch.einsum("pyxi,iodk->pyxdko", X.abs(), W1.abs()) + c1b.double().abs())
    if not s1_after_norm:
        u = u + S1_
        e_u = e_u + U32 * u.abs()
    n1, e_n = DC._ln64(u, e_u, lw.double(), lb.double(), 1e-6)
    if s1_after_norm:
        n1 = n1 + S1_
    g1 = DC.gelu64(n1)
    e_1 = 1.13 * e_n + 8 * U32 * (g1.abs() + n1.abs())                           # |gelu'| <= 1.13; erff and the products
    e_1 = e_1 + round16(g1, e_1)
    c = torch.einsum("pyxdki,ioel->pyxdkelo", g1, W2) + c2b.double()            # [P,g,g,2,2,2,2,32]
    e_c = torch.einsum("pyxdki,ioel->pyxdkelo", e_1, W2.abs()) + (64 + 2) * U32 * (torch.einsum("pyxdki,ioel->pyxdkelo", g1.abs(), W2.abs())
                                                                                    + c2b.double().abs())
    if not s0_after_gelu:
        c = c + S0_
        e_c = e_c + U32 * c.abs()
    g2 = DC.gelu64(c)
    e_2 = 1.13 * e_c + 8 * U32 * (g2.abs() + c.abs())
    e_2 = e_2 + round16(g2, e_2)
    if s0_after_gelu:
        g2 = g2 + S0_
    H = hyper.double()
    m = torch.einsum("pmo,pyxdkelo->pmydexkl", H, g2)                           # [P,m,g,2,2,g,2,2]
    e_m = torch.einsum("pmo,pyxdkelo->pmydexkl", H.abs(), e_2) + (32 + 2) * U32 * torch.einsum("pmo,pyxdkelo->pmydexkl", H.abs(), g2.abs())
    shape = (P, H.shape[1], 4 * g, 4 * g)
    return m.reshape(shape), (e_m + 4 * U32).reshape(shape)
