"""Shared cases, twins, fp64 restatements and bars for tests/test_sam_decoder_cpu.py and tests/test_gpu_sam_decoder.py.

Whole decoder: D1..D3 on the encoder cases' configurations with 256 channels (sam_cases.weights(name, 256)); the embedding is
N(0,1) [1,256,g,g] from generator seed 5, rounded to fp16.  Truth is gaussmart_amd.sam.decode_host in fp64 on the CPU, the
yardstick e16 the same modules in fp16 on the CPU, taken separately for the masks and for the IoU; bar = 2 x e16 (the two
formulations round at different points and each is a single draw).  The variants (no image positional embedding, no padding
token, no no_mask_embed, no point_embed[1]) must move the fp64 output by more than 10 x bar, and so must neighbouring points.

Stages: fp64 restatements of SD_PROMPT, SD_T2I, SD_I2T and SD_UP (include/gsr.h) from the same fp16-rounded inputs, with bars
built from the roundings the rules state."""
import functools
import math
import os

import numpy as np
import torch

import sam_cases as SC
from sam_cases import U16, U32, TINY16, round16
from gaussmart_amd import sam as S

# name -> (encoder case, points per side of the grid, how many of its points)
DECODER_CASES = {"D1": ("E1", 3, 9), "D2": ("E2", 3, 9), "D3": ("E3", 9, 67)}


def weights(name):
    return SC.weights(DECODER_CASES[name][0], 256)


@functools.lru_cache(maxsize=None)
def embedding(name):
    g = weights(name).config.grid
    return torch.randn(1, 256, g, g, generator=torch.Generator().manual_seed(5)).to(torch.float16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def points(name):
    _, side, n = DECODER_CASES[name]
    S_ = weights(name).config.image_size
    return S.point_grid(side, (S_ - 8, S_))[:n].contiguous()


def _without(w, key):
    return w.copy(replace={key: torch.zeros_like(w.tensors[key])})


@functools.lru_cache(maxsize=None)
def twin(name, dtype=torch.float64, variant="plain"):
    """(low_res [P,3,4g,4g], iou [P,3]) as fp64, of decode_host in `dtype` on the CPU (computed once per session)."""
    w, emb, pts = weights(name), embedding(name), points(name)
    if variant == "no_mask_embed":
        w = _without(w, "prompt_encoder.no_mask_embed.weight")
    elif variant == "no_point_embed":
        w = _without(w, "prompt_encoder.point_embed.1.weight")
    modules = S.host_decoder(w, dtype, "cpu")
    wide = torch.zeros_like(modules[2]) if variant == "no_pe" else None
    if variant == "no_pad":         # the prompt encoder's point token alone: 6 tokens per point
        prompt, decoder, own = modules
        with torch.no_grad():
            sparse, dense = prompt(pts.to(dtype)[None, :, None, :], torch.ones(1, len(pts), 1, dtype=torch.int64), None, None)
            low, iou = decoder(image_embeddings=emb.to(dtype), image_positional_embeddings=own, sparse_prompt_embeddings=sparse[:, :, :1],
                               dense_prompt_embeddings=dense, multimask_output=True)
        return low[0].double(), iou[0].double()
    low, iou = S.decode_host(w, emb, wide, pts, dtype, "cpu", modules)
    return low.double(), iou.double()


@functools.lru_cache(maxsize=None)
def model_bars(name):
    low64, iou64 = twin(name)
    low16, iou16 = twin(name, torch.float16)
    e_mask, e_iou = float((low16 - low64).abs().max()), float((iou16 - iou64).abs().max())
    out = {"e16_mask": e_mask, "e16_iou": e_iou, "bar_mask": 2 * e_mask, "bar_iou": 2 * e_iou}
    for variant in ("no_pe", "no_pad", "no_mask_embed", "no_point_embed"):
        lo, io = twin(name, variant=variant)
        out[variant + "_mask"], out[variant + "_iou"] = float((lo - low64).abs().max()), float((io - iou64).abs().max())
    out["neighbours"] = float((low64[1:] - low64[:-1]).flatten(1).abs().max(1).values.min())
    return out


def check_bar_conditions(b):
    assert b["e16_mask"] < 3e-2 and b["e16_iou"] < 1e-2, b              # the yardsticks themselves are small
    assert b["no_pe_mask"] > 10 * b["bar_mask"] and b["no_pe_iou"] > 10 * b["bar_iou"], b
    for variant in ("no_pad", "no_mask_embed", "no_point_embed"):
        assert b[variant + "_mask"] > 10 * b["bar_mask"], (variant, b)
    assert b["neighbours"] > 10 * b["bar_mask"], b                      # points that got mixed up must show


# ---------------------------------------------------------------- the scan of the generator test (tests/test_gpu_sam.py's recipe)
def tiny_scan(root, n_points=200):
    """A scan directory with two 96x128 pictures, 200 points in front of two cameras, as sam_cli and segment_cli read it."""
    from PIL import Image
    from gaussmart_amd import segment_cli
    rng = np.random.default_rng(5)
    os.makedirs(os.path.join(root, "images"))
    yy, xx = np.mgrid[0:96, 0:128]
    for i in range(2):
        img = np.stack([(xx * 2 + 40 * i) % 256, (yy * 2) % 256, ((xx // 16 + yy // 16) % 2) * 200], -1).astype(np.uint8)
        img[20:60, 30 + 20 * i:90] = (250, 30, 30)
        Image.fromarray(img).save(os.path.join(root, "images", f"{i:04d}.png"))
    pts = np.concatenate([rng.uniform(-0.5, 0.5, (n_points, 2)), rng.uniform(2.0, 3.0, (n_points, 1))], 1)
    segment_cli.write_cloud_ply(os.path.join(root, "points.ply"), pts, np.full((n_points, 3), 200, np.uint8))
    mats = {}
    for i in range(2):
        world = np.eye(4)
        world[0, 3] = 0.1 * i
        mats[f"world_mat_{i}"], mats[f"scale_mat_{i}"] = world, np.eye(4)
        mats[f"camera_mat_{i}"] = np.array([[1200.0, 0, 800, 0], [0, 1200.0, 600, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    np.savez(os.path.join(root, "cameras.npz"), **mats)
    return pts


# ---------------------------------------------------------------- fp64 restatements of the stage rules
def h16(shape, gen, scale=1.0):
    return (scale * torch.randn(shape, generator=gen)).to(torch.float16)


def prompt64(pts, S_, G, point1, nap, padding_as_point=False):
    """SD_PROMPT in fp64 -> (out [P,2,256], bar).  The bar follows the rule's fp32 roundings: the argument's error times 1 (the
    slope of sin and cos), the function's own (2 ulp of a value <= 1), and the addition of point_embed[1]."""
    p, G64 = pts.double(), G.double()
    a = 2 * ((p + 0.5) / S_) - 1
    arg = 2 * math.pi * (a @ G64)
    tok = torch.cat([torch.sin(arg), torch.cos(arg)], -1) + point1.double().reshape(1, 256)
    # a: three roundings of values <= 2 (sum, quotient, 2 x - 1); the two products and their sum; the product with fp32(2 pi)
    e_a = 6 * U32
    e_arg = 2 * math.pi * (e_a * G64.abs().sum(0, keepdim=True) + 3 * U32 * (a.abs() @ G64.abs())) + 4 * U32 * arg.abs()
    e_arg = torch.cat([e_arg, e_arg], -1)
    bar0 = e_arg + 4 * U32 + 2 * U32 * (tok.abs() + 1)
    second = nap.double().reshape(1, 256).expand(len(p), 256)
    if padding_as_point:            # the wrong reading: the padding point (0, 0), unshifted, encoded like a point
        arg0 = 2 * math.pi * (torch.full((1, 2), -1.0, dtype=torch.float64) @ G64)
        second = torch.cat([torch.sin(arg0), torch.cos(arg0)], -1).expand(len(p), 256)
    return torch.stack([tok, second], 1), torch.stack([bar0, torch.full_like(bar0, U32)], 1)


def t2i64(q, kx, kpe, v, shared, scale=0.25):
    """SD_T2I's attention in fp64 from the inputs as given -> (out [P,n,128], bar).  q f32 [P,n,128], n tokens per point (7
    for SAM, 8 for SAM2); kx, v fp16 [T,128] or [P,T,128]; kpe f32 [T,128] or None."""
    P, n = q.shape[:2]
    k = kx.double() + (0 if kpe is None else kpe.double())
    v = v.double()
    if shared:
        k, v = k[None].expand(P, -1, -1), v[None].expand(P, -1, -1)
    T = k.shape[1]
    qh = q.double().reshape(P, n, 8, 16).permute(0, 2, 1, 3)                # [P,8,n,16]
    kh, vh = (x.reshape(P, T, 8, 16).permute(0, 2, 1, 3) for x in (k, v))   # [P,8,T,16]
    dots = qh @ kh.transpose(-1, -2)
    s = dots * scale
    p = torch.softmax(s, -1)
    o = p @ vh
    mag = (qh.abs() @ kh.abs().transpose(-1, -2)) * scale
    es = (16 + 2) * U32 * mag + 2 * U32 * s.abs()       # the key's addition, the chain of 16, the scale
    spread = (s.max(-1, keepdim=True).values - s).max(-1, keepdim=True).values
    delta = 2 * es.max(-1, keepdim=True).values + 4 * U32 * (1 + spread)    # expf: 2 ulp, and its argument's rounding
    A = p @ vh.abs()
    e = (2 * delta + 2 * (T // 256 + 20) * U32) * A     # numerator and l: T / 256 additions per thread, 6 + 3 in the tree, the quotient
    bar = e + round16(o, e)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(P, n, 128)
    return back(o), back(bar)


def _ln64(y, ey, gamma, beta, eps):
    """LayerNorm over the last axis in fp64 and the first-order bound of its error for an input error ey >= 0, plus the
    rule's own fp32 roundings (DN_NORM's formula over n values)."""
    n = y.shape[-1]
    mu = y.mean(-1, keepdim=True)
    var = ((y - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    yh = (y - mu) * rstd
    ey = ey + (math.log2(n) + n / 64 + 8) * U32 * y.abs().max(-1, keepdim=True).values
    eh = rstd * (ey + ey.mean(-1, keepdim=True) + yh.abs() * (yh.abs() * ey).mean(-1, keepdim=True))
    out = yh * gamma + beta
    return out, eh * gamma.abs() + 4 * U32 * ((yh * gamma).abs() + beta.abs())


def i2t64(qx, qpe, k, v, x, shared, ow, ob, lw, lb, norm=True, eps=1e-6):
    """SD_I2T in fp64 -> (stream [P,T,256], bar).  k, v f32 [P,n,128], n tokens per point; eps: layer_norm4's (SAM2's is 1e-5).
    norm=False: layer_norm4 left out (the wrong reading)."""
    P, n = k.shape[:2]
    q = qx.double() + qpe.double()
    x = x.double()
    if shared:
        q, x = q[None].expand(P, -1, -1), x[None].expand(P, -1, -1)
    T = q.shape[1]
    qh = q.reshape(P, T, 8, 16).permute(0, 2, 1, 3)                          # [P,8,T,16]
    kh, vh = (t.double().reshape(P, n, 8, 16).permute(0, 2, 1, 3) for t in (k, v))
    s = (qh @ kh.transpose(-1, -2)) * 0.25
    p = torch.softmax(s, -1)
    ctx = (p @ vh).permute(0, 2, 1, 3).reshape(P, T, 128)
    mag = (qh.abs() @ kh.abs().transpose(-1, -2)) * 0.25
    delta = 2 * ((18 * U32 * mag + 2 * U32 * s.abs()).max(-1, keepdim=True).values) + 8 * U32
    e_ctx = ((2 * delta + 20 * U32) * (p @ vh.abs())).permute(0, 2, 1, 3).reshape(P, T, 128)
    e_ctx = e_ctx + round16(ctx, e_ctx)                                     # ctx is ROUNDED TO fp16
    W = ow.double()
    a = ctx @ W.T + ob.double()
    e_a = e_ctx @ W.abs().T + (128 + 2) * U32 * (ctx.abs() @ W.abs().T + ob.double().abs())
    y = x + a
    e_y = e_a + U32 * y.abs()
    if not norm:
        return y, e_y + round16(y, e_y)
    out, e = _ln64(y, e_y, lw.double(), lb.double(), eps)
    return out, e + round16(out, e)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def up64(x, g, c1w, c1b, lw, lb, c2w, c2b, hyper, swap1=False, swap2=False):
    """SD_UP in fp64 from the module's own tensors -> (low_res [P,m,4g,4g], bar).  x fp16 [P,T,256]; c1w [256,64,2,2], c2w
    [64,32,2,2] as ConvTranspose2d holds them; hyper f32 [P,m,32].  swap1 / swap2: the (dy, dx) taps of that convolution
    transposed (the wrong reading)."""
    P = x.shape[0]
    X = x.double().reshape(P, g, g, 256)
    W1, W2 = c1w.double(), c2w.double()
    if swap1:
        W1 = W1.transpose(2, 3)
    if swap2:
        W2 = W2.transpose(2, 3)
    u = torch.einsum("pyxi,iodk->pyxdko", X, W1) + c1b.double()                 # [P,g,g,2,2,64]
    e_u = (256 + 2) * U32 * (torch.einsum("pyxi,iodk->pyxdko", X.abs(), W1.abs()) + c1b.double().abs())
    n1, e_n = _ln64(u, e_u, lw.double(), lb.double(), 1e-6)
    g1 = gelu64(n1)
    e_1 = 1.13 * e_n + 8 * U32 * (g1.abs() + n1.abs())                           # |gelu'| <= 1.13; erff and the products
    e_1 = e_1 + round16(g1, e_1)
    c = torch.einsum("pyxdki,ioel->pyxdkelo", g1, W2) + c2b.double()            # [P,g,g,2,2,2,2,32]
    e_c = torch.einsum("pyxdki,ioel->pyxdkelo", e_1, W2.abs()) + (64 + 2) * U32 * (torch.einsum("pyxdki,ioel->pyxdkelo", g1.abs(), W2.abs())
                                                                                    + c2b.double().abs())
    g2 = gelu64(c)
    e_2 = 1.13 * e_c + 8 * U32 * (g2.abs() + c.abs())
    e_2 = e_2 + round16(g2, e_2)
    H = hyper.double()
    m = torch.einsum("pmo,pyxdkelo->pmydexkl", H, g2)                           # [P,m,g,2,2,g,2,2]
    e_m = torch.einsum("pmo,pyxdkelo->pmydexkl", H.abs(), e_2) + (32 + 2) * U32 * torch.einsum("pmo,pyxdkelo->pmydexkl", H.abs(), g2.abs())
    shape = (P, H.shape[1], 4 * g, 4 * g)
    return m.reshape(shape), (e_m + 4 * U32).reshape(shape)
