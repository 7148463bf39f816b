"""Shared weights, inputs, twins and bars for tests/test_sam_cpu.py and tests/test_gpu_sam.py.

Weights: gaussmart_amd.sam.random_sam_weights' recipe (default initialisation is useless: the twin's output comes out around
1e-20 with it).  64 output channels for the encoder cases (no decoder); the generator case has 256.  pixel_values: N(0, 1)
rounded to fp16.

The independent twin is transformers' own SamVisionEncoder on the CPU holding the same tensors (gaussmart_amd.sam.sam_host),
in fp64 (the truth), in fp16 (the library's own formulation: its error is the yardstick of the whole-encoder bar), and in fp64
with the relative-position bias removed or with the padded keys of the windows masked (the bar must be far below what
either changes).

The mask cases: cones a (r - d) / r plus 0.7 x up-sampled noise, mask 0 constant -5 (empty), mask 1 constant +5 (full)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from gaussmart_amd import sam as S

U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY16 = 2.0 ** -25

# name -> (hidden, heads, layers, global layers, window, image)
ENCODER_CASES = {"E1": (128, 2, 2, (1,), 3, 112), "E2": (320, 4, 2, (1,), 4, 144), "E3": (128, 2, 3, (2,), 14, 272)}


def config(name, channels=64):
    hidden, heads, layers, glob, window, image = ENCODER_CASES[name]
    return S.SamConfig(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, mlp_dim=4 * hidden, window_size=window,
                       global_attn_indexes=glob, output_channels=channels, image_size=image)


@functools.lru_cache(maxsize=None)
def weights(name, channels=64):
    return S.random_sam_weights(config(name, channels), seed=4321 + channels)


@functools.lru_cache(maxsize=None)
def pixels(name):
    S_ = ENCODER_CASES[name][5]
    g = torch.Generator().manual_seed(S_)
    return torch.randn(3, S_, S_, generator=g).to(torch.float16).to(torch.float32)


def _mask_padded(model, g):
    """The windowed layers' attention with the padded keys at -inf (what a wrong reading of the padding would compute)."""
    for layer in model.layers:
        w = layer.window_size
        if w == 0:
            continue
        nw = -(-g // w)
        inside = torch.arange(nw * w) < g
        pad = ~(inside[:, None] & inside[None, :]).reshape(nw, w, nw, w).permute(0, 2, 1, 3).reshape(nw * nw, w * w)

        def forward(hidden_states, output_attentions=None, attn=layer.attn, pad=pad):
            b, h, wd, _ = hidden_states.shape
            nh = attn.num_attention_heads
            qkv = attn.qkv(hidden_states).reshape(b, h * wd, 3, nh, -1).permute(2, 0, 3, 1, 4)
            q, k, v = qkv.reshape(3, b * nh, h * wd, -1).unbind(0)
            a = (q * attn.scale) @ k.transpose(-2, -1)
            a = a + attn.get_decomposed_rel_pos(q, attn.rel_pos_h, attn.rel_pos_w, (h, wd), (h, wd)).reshape_as(a)
            a = torch.softmax(a.masked_fill(pad.repeat_interleave(nh, 0)[:, None, :], float("-inf")), -1)
            out = (a @ v).reshape(b, nh, h, wd, -1).permute(0, 2, 3, 1, 4).reshape(b, h, wd, -1)
            return attn.proj(out), None
        layer.attn.forward = forward
    return model


@functools.lru_cache(maxsize=None)
def twin(name, dtype=torch.float64, variant="plain"):
    """[C,g,g] of pixels(name) through the library's encoder in `dtype` on the CPU, as fp64 (computed once per session)."""
    w = weights(name)
    model = S.host_encoder(w, dtype, "cpu")
    if variant == "no_rel":
        with torch.no_grad():
            for layer in model.layers:
                layer.attn.rel_pos_h.zero_()
                layer.attn.rel_pos_w.zero_()
    elif variant == "masked_pad":
        model = _mask_padded(model, w.config.grid)
    return S.sam_host(w, pixels(name), dtype, "cpu", model).double()


@functools.lru_cache(maxsize=None)
def model_bars(name):
    """bar = 2 x the max-abs error of the library's fp16 model against its fp64 model on the same inputs (the factor 2: the
    two formulations round at different points and each is a single draw)."""
    o64, o16 = twin(name), twin(name, torch.float16)
    e16 = float((o16 - o64).abs().max())
    return {"bar": 2 * e16, "e16": e16, "no_rel": float((twin(name, variant="no_rel") - o64).abs().max()),
            "masked_pad": float((twin(name, variant="masked_pad") - o64).abs().max())}


def check_bar_conditions(b):
    assert b["e16"] < 1e-2, b                       # the yardstick itself is small
    assert b["no_rel"] > 10 * b["bar"], b           # a missing relative-position bias cannot hide
    assert b["masked_pad"] > 10 * b["bar"], b       # nor can padded keys that were left out


def round16(v, e=0.0):
    return U16 * (v.abs() + e) + TINY16


# ---------------------------------------------------------------- SV_ATTN in fp64
def attention64(qkv, bias, Rh, Rw, g, w, heads, hd):
    """fp64 (out [T,hidden], bar [T,hidden]) of the SV_ATTN rule from fp16 inputs, padded keys and both bias terms included.
    The bar follows the rule's stated roundings, as DN_ATTN's does (tests/test_gpu_dino.py), with the three extra fp32
    roundings of the score (two bias additions, the log2 e product) and the bias chains' own error."""
    s = g if w == 0 else w
    nw = -(-g // s)
    hidden = heads * hd
    P = nw * s
    full = bias.double().reshape(1, 1, 3 * hidden).repeat(P, P, 1)             # what DN_LINEAR gives on a zero row
    full[:g, :g] = qkv.double().reshape(g, g, 3 * hidden)
    win = full.reshape(nw, s, nw, s, 3, heads, hd).permute(0, 2, 4, 5, 1, 3, 6).reshape(nw * nw, 3, heads, s * s, hd)
    q, k, v = win[:, 0], win[:, 1], win[:, 2]                                   # [W,heads,s s,hd]
    idx = torch.arange(s)[:, None] - torch.arange(s)[None, :] + s - 1
    RH, RW = Rh.double()[idx], Rw.double()[idx]                                # [s(q),s(k),hd]
    q5 = q.reshape(nw * nw, heads, s, s, hd)
    rh = torch.einsum("bnhwc,hkc->bnhwk", q5, RH)
    rw = torch.einsum("bnhwc,wkc->bnhwk", q5, RW)
    arh = torch.einsum("bnhwc,hkc->bnhwk", q5.abs(), RH.abs())
    arw = torch.einsum("bnhwc,wkc->bnhwk", q5.abs(), RW.abs())
    scale = hd ** -0.5
    qk = q @ k.transpose(-1, -2)
    rel = (rh[..., :, None] + rw[..., None, :]).reshape(nw * nw, heads, s * s, s * s)
    t = qk * scale + rel
    p = torch.softmax(t, -1)
    o = p @ v
    mag = (qk.abs() * scale + (rh.abs()[..., :, None] + rw.abs()[..., None, :]).reshape_as(qk))
    chain = hd * U32 * ((q.abs() @ k.abs().transpose(-1, -2)) * scale + (arh[..., :, None] + arw[..., None, :]).reshape_as(qk))
    es = chain + 6 * U32 * mag          # scale product (and the constant's rounding), two additions, log2 e (and its rounding)
    spread = (t.max(-1, keepdim=True).values - t).max(-1, keepdim=True).values
    delta = 2 * es.max(-1, keepdim=True).values + U32 * spread + 4 * U32
    A = p @ v.abs()
    T = s * s
    e = (U16 + 2 * delta + (4 * T + 16) * U32) * A + TINY16 * v.abs().sum(-2, keepdim=True)
    bar = e + round16(o, e)

    def back(x):        # [W,heads,s s,hd] -> [T,hidden] of the real tokens
        x = x.reshape(nw, nw, heads, s, s, hd).permute(0, 3, 1, 4, 2, 5).reshape(P, P, hidden)
        return x[:g, :g].reshape(g * g, hidden)
    return back(o), back(bar)


# ---------------------------------------------------------------- mask logits
@functools.lru_cache(maxsize=None)
def mask_logits(L, in_h, in_w, n=24, amp=(2.0, 12.0), seed=0):
    """f32 [n,L,L]: cones centred inside the input region plus 0.7 x bilinear-up-sampled N(0,1) noise on an L/4 grid; mask 0
    is constant -5, mask 1 constant +5.  The amplitudes are spread evenly over `amp` (in a seeded order)."""
    g = torch.Generator().manual_seed(1000 * L + 7 * n + seed)
    ys, xs = torch.meshgrid(torch.arange(L, dtype=torch.float32), torch.arange(L, dtype=torch.float32), indexing="ij")
    a = torch.linspace(amp[0], amp[1], n)[torch.randperm(n, generator=g)]
    cy = torch.rand(n, generator=g) * (in_h / 4.0)
    cx = torch.rand(n, generator=g) * (in_w / 4.0)
    r = L * (0.125 + 0.375 * torch.rand(n, generator=g))
    d = torch.sqrt((ys[None] - cy[:, None, None]) ** 2 + (xs[None] - cx[:, None, None]) ** 2)
    cone = a[:, None, None] * (r[:, None, None] - d) / r[:, None, None]
    noise = F.interpolate(torch.randn(n, 1, L // 4, L // 4, generator=g), (L, L), mode="bilinear", align_corners=False)[:, 0]
    out = cone + 0.7 * noise
    out[0] = -5.0
    out[1] = 5.0
    return out.contiguous()


def mask_truth(logits, input_size, mask_size, tau=0.0, delta=1.0, chunk=25):
    """The fp64 torch formulation, reduced per mask: dict of on (bool [n,h,w]: value > tau), decided (bool [n,h,w]), and the
    fp64 counts area / inter / union.  decided: the fp64 value is more than 32 x 2^-24 x max|logit| from tau - delta, tau and
    tau + delta."""
    eps = 32 * U32 * float(logits.abs().max())
    on, decided, counts = [], [], []
    for part in logits.split(chunk):
        v = S.upsample_host(part, input_size, mask_size, torch.float64)
        on.append(v > tau)
        decided.append(((v - (tau - delta)).abs() > eps) & ((v - tau).abs() > eps) & ((v - (tau + delta)).abs() > eps))
        counts.append(torch.stack([(v > tau).flatten(1).sum(1), (v > tau + delta).flatten(1).sum(1), (v > tau - delta).flatten(1).sum(1)], 1))
    return {"on": torch.cat(on), "decided": torch.cat(decided), "counts": torch.cat(counts)}


# ---------------------------------------------------------------- SM_NMS as a plain loop
def nms_loop(boxes, scores, keep_in, theta):
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    cand = [i for i in range(len(scores)) if (keep_in is None or keep_in[i]) and not np.isnan(scores[i])]
    cand.sort(key=lambda i: (-scores[i], i))
    b = boxes[cand]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(len(cand), bool)
    kept = []
    with np.errstate(all="ignore"):
        for i in range(len(cand)):
            if dead[i]:
                continue
            kept.append(cand[i])
            w = np.maximum(np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]), np.float32(0))
            h = np.maximum(np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]), np.float32(0))
            inter = w * h
            dead[i + 1:] |= inter / (area[i] + area[i + 1:] - inter) > np.float32(theta)
    return kept


def random_boxes(n, seed, extent=200.0, clustered=False):
    g = torch.Generator().manual_seed(seed)
    if clustered:
        centres = extent * torch.rand(max(1, n // 40), 2, generator=g)
        c = centres[torch.randint(len(centres), (n,), generator=g)] + 2.0 * torch.randn(n, 2, generator=g)
    else:
        c = extent * torch.rand(n, 2, generator=g)
    wh = 4.0 + 30.0 * torch.rand(n, 2, generator=g)
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1).round()
    scores = (torch.randint(0, max(2, n // 3), (n,), generator=g).float() / max(2, n // 3))       # many ties
    return boxes.contiguous(), scores.contiguous()
