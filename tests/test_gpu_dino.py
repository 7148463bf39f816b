"""The DINOv3 ViT kernels (csrc/dino.hip, csrc/vit.hip; include/gsr.h: DN_EMBED, DN_NORM, DN_LINEAR, DN_ROPE, DN_ATTN, DN_POOL, DN_COS) on
the device, everything through the C ABI: each stage against fp64 from the same fp16 inputs with a bar that follows the
roundings its rule states, the whole model against transformers' fp64 model with a bar measured on transformers' own fp16
model, the bit-equalities the rules promise, the refusals, and train_cli with --dino_dir.  Weights, images, twins and the bar
arithmetic are in tests/dino_cases.py.  GSR_DINO_PARITY_REPORT=<file>: the measured errors and bars are appended there
(profiles/dino_parity.txt is such a run)."""
import csv
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_cases as DC
from dino_cases import U16, U32, TINY16
from gaussmart_amd import _lib
from gaussmart_amd import dino as D
from gaussmart_amd._dev import ptr, stream, workspace
from gaussmart_amd.loss_utils import dino_loss

pytestmark = pytest.mark.gpu

# the four GEMM shapes of configs A and C (K, N), and the token counts of the three image sizes
GEMMS = [(128, 128), (128, 512), (512, 128), (768, 768), (768, 3072), (3072, 768)]
TOKENS = [20, 131, 277]


def report(line):
    out = os.environ.get("GSR_DINO_PARITY_REPORT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


def held(name, got, want64, bar):
    """max over the elements of |got - want| / bar must be <= 1; the figure is reported before it is asserted."""
    err = (got.detach().double().cpu() - want64).abs()
    use = float((err / bar).max())
    report(f"{name}: max err {float(err.max()):.3e}, max bar {float(torch.as_tensor(bar).max()):.3e}, worst err/bar {use:.3f}")
    assert torch.isfinite(got).all() and use <= 1.0, (name, use)


def h16(shape, g, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(torch.float16)


# ---------------------------------------------------------------- DN_LINEAR
def linear_dev(x, w, b, epi, lam=None, resid=None):
    M, K = x.shape
    N = w.shape[0]
    out = resid.clone() if resid is not None else torch.full((M, N), float("nan"), dtype=torch.float16, device=x.device)
    _lib.check(_lib.lib().gsr_dino_linear(ptr(x), ptr(w), ptr(b), ptr(lam), M, K, N, epi, ptr(out), stream(x.device)))
    return out


@pytest.mark.parametrize("K,N", GEMMS)
@pytest.mark.parametrize("T", TOKENS)
def test_linear_epilogues_against_fp64(gpu_device, T, K, N):
    g = torch.Generator().manual_seed(T * 7 + K + 3 * N)
    x, w, b = h16((T, K), g), h16((N, K), g, K ** -0.5), h16((N,), g, 0.1)
    lam, resid = (0.5 + torch.rand(N, generator=g)).to(torch.float16), torch.randn(T, N, generator=g)
    dx, dw, db, dl = (t.to(gpu_device) for t in (x, w, b, lam))
    u, S, E = DC.linear_bars(x, w, b)
    # + bias, rounded to fp16 (and the same without a bias: k_proj)
    held(f"linear bias T{T} K{K} N{N}", linear_dev(dx, dw, db, _lib.GSR_DINO_EPI_BIAS), u, E + DC.round16(u, E))
    u0, _, E0 = DC.linear_bars(x, w, None)
    held(f"linear nobias T{T} K{K} N{N}", linear_dev(dx, dw, None, _lib.GSR_DINO_EPI_BIAS), u0, E0 + DC.round16(u0, E0))
    # exact GELU: |gelu'| <= 1.13 carries E; erff and the three fp32 products: 8 roundings of fp32 on |gelu| + |u|
    gl = DC.gelu64(u)
    Eg = 1.13 * E + 8 * U32 * (gl.abs() + u.abs())
    held(f"linear gelu T{T} K{K} N{N}", linear_dev(dx, dw, db, _lib.GSR_DINO_EPI_GELU), gl, Eg + DC.round16(gl, Eg))
    # LayerScale + residual in fp32: resid + lambda (acc + bias), one more fp32 rounding (the fma's)
    r = resid.double() + lam.double() * u
    Er = lam.double().abs() * E
    held(f"linear resid T{T} K{K} N{N}", linear_dev(dx, dw, db, _lib.GSR_DINO_EPI_RESID, dl, resid.to(gpu_device)), r, Er + U32 * (r.abs() + Er))


# ---------------------------------------------------------------- DN_NORM
@pytest.mark.parametrize("hidden", [128, 768])
@pytest.mark.parametrize("T", TOKENS)
def test_norm_against_fp64(gpu_device, T, hidden):
    g = torch.Generator().manual_seed(T + hidden)
    x = 3.0 * torch.randn(T, hidden, generator=g) + 1.0
    gam, beta = (0.5 + torch.rand(hidden, generator=g)).to(torch.float16), h16((hidden,), g, 0.1)
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    z = d * rstd * gam.double()
    y = z + beta.double()
    # fp32: the mean's sum (n additions on |x|), the variance's sum (n additions, plus the mean's error in every d), rsqrt,
    # two products, one addition
    dmean = hidden * U32 * x64.abs().mean(1, keepdim=True)
    var_rel = (hidden + 8) * U32 + 2 * dmean * d.abs().mean(1, keepdim=True) / var
    e32 = z.abs() * (0.5 * var_rel + 6 * U32) + dmean * rstd * gam.double().abs() + U32 * y.abs()
    L = _lib.lib()
    dx, dg, db = x.to(gpu_device), gam.to(gpu_device), beta.to(gpu_device)
    for out_f32, dtype in ((0, torch.float16), (1, torch.float32)):
        out = torch.full((T, hidden), float("nan"), dtype=dtype, device=gpu_device)
        _lib.check(L.gsr_dino_norm(ptr(dx), T, hidden, hidden, ptr(dg), ptr(db), 1e-5, out_f32, ptr(out), stream(gpu_device)))
        held(f"norm f{32 if out_f32 else 16} T{T} h{hidden}", out, y, e32 + (0.0 if out_f32 else DC.round16(y, e32)))
    # the pooled form: B rows, T hidden apart, are the same bits as those rows of the full call
    full = torch.empty(T, hidden, device=gpu_device)
    _lib.check(L.gsr_dino_norm(ptr(dx), T, hidden, hidden, ptr(dg), ptr(db), 1e-5, 1, ptr(full), stream(gpu_device)))
    rows = torch.empty(2, hidden, device=gpu_device)
    _lib.check(L.gsr_dino_norm(ptr(dx), 2, hidden, 10 * hidden, ptr(dg), ptr(db), 1e-5, 1, ptr(rows), stream(gpu_device)))
    assert torch.equal(rows, full[[0, 10]])


# ---------------------------------------------------------------- DN_ROPE
@pytest.mark.parametrize("Hp,Wp", [(3, 5), (9, 14), (17, 16)])
def test_rope_against_fp64(gpu_device, Hp, Wp):
    heads, prefix, B = 2, 5, 2
    T = prefix + Hp * Wp
    g = torch.Generator().manual_seed(Hp * Wp)
    q, k = h16((B, T, heads * 64), g), h16((B, T, heads * 64), g)
    cos, sin = D.rope_table(Hp, Wp, 100.0)

    def want(t):
        t64 = t.double().reshape(B, T, heads, 64)
        p = t64[:, prefix:]
        rot = torch.cat([-p[..., 32:], p[..., :32]], -1)
        c, s = cos[None, :, None, :], sin[None, :, None, :]
        out = t64.clone()
        out[:, prefix:] = p * c + rot * s
        # fp32 angle (coordinate, power, two products: 8 roundings on an angle below 2 pi) -> sin / cos within 64 x 2^-24;
        # then two fp32 products and an addition, and one rounding to fp16
        e = 64 * U32 * (p.abs() + rot.abs()) + 3 * U32 * ((p * c).abs() + (rot * s).abs())
        bar = torch.zeros_like(t64)
        bar[:, prefix:] = e + DC.round16(out[:, prefix:], e)
        return out.reshape(B, T, -1), bar.reshape(B, T, -1)

    dq, dk = q.to(gpu_device), k.to(gpu_device)
    _lib.check(_lib.lib().gsr_dino_rope(ptr(dq), ptr(dk), B, T, heads, Hp, Wp, 100.0, stream(gpu_device)))
    for name, dev, host in (("q", dq, q), ("k", dk, k)):
        w64, bar = want(host)
        assert torch.equal(dev[:, :prefix].cpu(), host[:, :prefix])          # CLS and registers are not rotated
        held(f"rope {name} {Hp}x{Wp}", dev[:, prefix:], w64[:, prefix:], bar[:, prefix:])
    # q alone gives the same q
    dq2 = q.to(gpu_device)
    _lib.check(_lib.lib().gsr_dino_rope(ptr(dq2), None, B, T, heads, Hp, Wp, 100.0, stream(gpu_device)))
    assert torch.equal(dq2, dq)


# ---------------------------------------------------------------- DN_ATTN
def attn_dev(q, k, v, B, T, heads):
    out = torch.full((B, T, heads * 64), float("nan"), dtype=torch.float16, device=q.device)
    _lib.check(_lib.lib().gsr_dino_attn(ptr(q), ptr(k), ptr(v), B, T, heads, ptr(out), stream(q.device)))
    return out


@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("T", TOKENS)
def test_attention_against_fp64(gpu_device, T, heads):
    B = 2
    g = torch.Generator().manual_seed(T + heads)
    q, k, v = h16((B, T, heads * 64), g), h16((B, T, heads * 64), g), h16((B, T, heads * 64), g)
    split = lambda t: t.double().reshape(B, T, heads, 64).permute(0, 2, 1, 3)         # [B,heads,T,64]
    q64, k64, v64 = split(q), split(k), split(v)
    s = q64 @ k64.transpose(-1, -2) / 8.0
    p = torch.softmax(s, -1)
    o = p @ v64
    # scores: 64-term fp32 chain on sum_d |q_d k_d| / 8, then ONE fp32 rounding of the product with log2(e) / 8 (the constant's own
    # rounding is another): 2 x 2^-24 |s| in the exponent's natural units; 2^(t - m): the score's error enters twice (t and the
    # maximum), the subtraction rounds |t - m| (2^-24 x spread), v_exp_f32 and the two neighbours 4 roundings: relative delta per
    # query row (the worst kv of the row)
    es = 64 * U32 * (q64.abs() @ k64.abs().transpose(-1, -2)) / 8.0 + 2 * U32 * s.abs()
    spread = (s.max(-1, keepdim=True).values - s).max(-1, keepdim=True).values
    delta = 2 * es.max(-1, keepdim=True).values + U32 * spread + 4 * U32
    A = p @ v64.abs()                                       # sum_j p_j |v_j|
    # P rounded to fp16 (relative 2^-11; below fp16's normals absolute 2^-25 per kv, against l >= 1), numerator and
    # denominator each carry delta; fp32 roundings: the P V chain and l's chain at most T each, per KV tile (T / 64 + 1 of them)
    # the rescale of both and exp(m_old - m_new) (6 each, so below 2 T + 15 in all), the division one: 4 T + 16
    e = (U16 + 2 * delta + (4 * T + 16) * U32) * A + TINY16 * v64.abs().sum(-2, keepdim=True)
    bar = e + DC.round16(o, e)
    got = attn_dev(q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), B, T, heads)
    held(f"attn T{T} heads{heads}", got.reshape(B, T, heads, 64).permute(0, 2, 1, 3), o, bar)
    # the KV tail contributes nothing: K and V rows past T (the buffer's padding) at 1e4 change no bit; nor does the batch
    pad = lambda t, fill: torch.cat([t[:1], torch.full((1, 64, heads * 64), fill, dtype=torch.float16)], 1).to(gpu_device)
    alone = attn_dev(q[:1].to(gpu_device), pad(k, 1e4), pad(v, 1e4), 1, T, heads)
    assert torch.equal(alone, got[:1])


# ---------------------------------------------------------------- DN_EMBED
def embed_dev(cfg, w, x, dev):
    B, _, H, W = x.shape
    L = _lib.lib()
    t = {k: v.to(dev) for k, v in w.tensors.items() if k.startswith("embeddings.")}
    nbytes = L.gsr_dino_embed_workspace_bytes(B, H, W)
    ws = workspace(nbytes, dev)
    out = torch.full((B, cfg.tokens(H, W), cfg.hidden_size), float("nan"), device=dev)
    c = cfg.to_c()
    xd = x.to(dev).contiguous()
    _lib.check(L.gsr_dino_embed(C.byref(c), ptr(xd), None, B, H, W, ptr(t["embeddings.cls_token"]), ptr(t["embeddings.register_tokens"]),
                                ptr(t["embeddings.patch_embeddings.weight"]), ptr(t["embeddings.patch_embeddings.bias"]), ptr(ws), nbytes,
                                ptr(out), stream(dev)))
    return out


@pytest.mark.parametrize("name,H,W", [("A", 48, 80), ("A", 144, 224), ("C", 272, 256), ("A", 56, 83)])
def test_embed_against_fp64(gpu_device, name, H, W):
    cfg, w = DC.config(name), DC.weights(name)
    x = DC.images(H, W)
    out = embed_dev(cfg, w, x, gpu_device)
    Hp, Wp, R = H // 16, W // 16, cfg.num_register_tokens
    # the constants as the kernel receives them (fp32), the arithmetic in fp64
    mean = torch.tensor(cfg.image_mean, dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor(cfg.image_std, dtype=torch.float32).double().view(1, 3, 1, 1)
    xn = (x.double()[:, :, :16 * Hp, :16 * Wp] - mean) / std
    pw, pb = w.tensors["embeddings.patch_embeddings.weight"].double(), w.tensors["embeddings.patch_embeddings.bias"].double()
    y = F.conv2d(xn, pw, pb, stride=16).flatten(2).transpose(1, 2)
    S = F.conv2d(xn.abs(), pw.abs(), None, stride=16).flatten(2).transpose(1, 2)
    # xn: a subtraction and a division in fp32, then ONE rounding to fp16; a 768-term fp32 chain; the bias addition in fp32
    held(f"embed {name} {H}x{W}", out[:, 1 + R:], y, (U16 + 3 * U32 + 768 * U32) * S + U32 * y.abs())
    assert torch.equal(out[:, 0].cpu(), w.tensors["embeddings.cls_token"].float().reshape(1, -1).expand(2, -1))
    assert torch.equal(out[:, 1:1 + R].cpu(), w.tensors["embeddings.register_tokens"].float().expand(2, -1, -1))


# ---------------------------------------------------------------- the whole model
def run_model(name, x, dev, registers=4, tokens=True, separate=False):
    enc = D.DINOImageEncoder(DC.weights(name, registers))
    if separate:
        return enc.forward([t.to(dev) for t in x], tokens=tokens)
    return enc.forward(x.to(dev), tokens=tokens)


@pytest.mark.parametrize("name,H,W", DC.MODEL_CASES)
def test_whole_model_against_the_fp64_twin(gpu_device, name, H, W):
    bars = DC.model_bars(name, H, W)
    DC.check_bar_conditions(bars)
    l64, p64 = DC.twin(name, H, W)
    pooled, last = run_model(name, DC.images(H, W), gpu_device)
    report(f"model {name} {H}x{W}: transformers fp16 vs fp64 {bars['e16'][0]:.3e} (tokens) {bars['e16'][1]:.3e} (pooled); without RoPE "
           f"{bars['no_rope'][0]:.3f} / {bars['no_rope'][1]:.3f}; cosine of the two images {bars['cos']:.3f}")
    held(f"model {name} {H}x{W} last_hidden", last, l64, bars["last"])
    held(f"model {name} {H}x{W} pooled", pooled, p64, bars["pooled"])
    assert torch.equal(pooled, last[:, 0])


def test_no_registers_against_the_twin(gpu_device):
    bars = {k: v for k, v in DC.model_bars("A", 48, 80).items()}
    l64, p64 = DC.twin("A", 48, 80, registers=0)
    l16, p16 = DC.twin("A", 48, 80, torch.float16, registers=0)
    pooled, last = run_model("A", DC.images(48, 80), gpu_device, registers=0)
    assert last.shape == (2, 16, 128)
    held("model A 48x80 registers=0 last_hidden", last, l64, 2 * float((l16 - l64).abs().max()))
    held("model A 48x80 registers=0 pooled", pooled, p64, 2 * float((p16 - p64).abs().max()))
    assert bars["e16"][0] < 1e-2


def test_bit_equalities(gpu_device):
    x = DC.images(56, 83)
    pooled, last = run_model("A", x, gpu_device)
    # trailing rows and columns are not read: 56x83 equals its 48x80 crop
    pc, lc = run_model("A", x[:, :, :48, :80].contiguous(), gpu_device)
    assert torch.equal(pooled, pc) and torch.equal(last, lc)
    # two runs are equal
    p2, l2 = run_model("A", x, gpu_device)
    assert torch.equal(pooled, p2) and torch.equal(last, l2)
    # an image alone equals the same image as either half of a pair (contiguous batch, separate allocations, swapped)
    for i in (0, 1):
        pa, la = run_model("A", x[i:i + 1], gpu_device)
        assert torch.equal(pa[0], pooled[i]) and torch.equal(la[0], last[i])
    ps, ls = run_model("A", [x[1], x[0]], gpu_device, separate=True)
    assert torch.equal(ps[0], pooled[1]) and torch.equal(ps[1], pooled[0]) and torch.equal(ls[0], last[1]) and torch.equal(ls[1], last[0])
    # across a tile boundary as well (T = 131)
    y = DC.images(144, 224)
    pb, lb = run_model("B", y, gpu_device)
    pa, la = run_model("B", y[1:2], gpu_device)
    assert torch.equal(pa[0], pb[1]) and torch.equal(la[0], lb[1])
    enc = D.DINOImageEncoder(DC.weights("B"))
    assert torch.equal(enc.encode_tensor(y[1].to(gpu_device)), pb[1]) and torch.equal(enc.encode_pair(y[0].to(gpu_device), y[1].to(gpu_device)), pb)
    assert torch.equal(enc.encode_tokens(y[0].to(gpu_device)), lb[0])


# ---------------------------------------------------------------- DN_COS and dino_loss
def test_cosine_and_dino_loss_against_fp64(gpu_device):
    g = torch.Generator().manual_seed(4)
    for n, lam in ((768, 0.05), (128, 0.1), (1000, 1.0), (3, 0.05)):
        a = 5 * torch.randn(n, generator=g)
        b = 0.5 * a + 4 * torch.randn(n, generator=g)
        lam16 = D.lambda_fp16(lam)
        a64, b64 = a.double(), b.double()
        v64 = lam16 * float(a64 @ b64 / (a64.norm() * b64.norm()))
        got = float(D.scaled_cosine(a.to(gpu_device), b.to(gpu_device), lam))
        # three n-term fp32 sums on non-negative terms (sum |a b| <= |a| |b|), two square roots, three products, a division
        bar = lam16 * (3 * (n + 8) * U32)
        report(f"cosine n{n} lambda {lam}: err {abs(got - v64):.3e}, bar {bar:.3e}")
        assert abs(got - v64) <= bar
    # dino_loss: the encoder's two pooled rows through DN_COS, rounded to fp16 once
    enc = D.DINOImageEncoder(DC.weights("A"))
    x = DC.images(48, 80).to(gpu_device)
    val = dino_loss(x[0], x[1], enc, 0.05)
    assert val.dtype == torch.float16 and val.dim() == 0 and not val.requires_grad
    pooled = enc.encode_pair(x[0], x[1]).double().cpu()
    v64 = D.lambda_fp16(0.05) * float(F.cosine_similarity(pooled[0], pooled[1], dim=0))
    assert abs(float(val) - v64) <= U16 * abs(v64) + 0.05 * 3 * (128 + 8) * U32
    zero = D.scaled_cosine(torch.zeros(8, device=gpu_device), torch.ones(8, device=gpu_device), 0.05)
    assert float(zero) == 0.0          # the 1e-8 floor, not a division by zero


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(gpu_device):
    L = _lib.lib()
    good = DC.config("A")
    x = torch.zeros(2, 3, 48, 80, device=gpu_device)
    pooled = torch.full((2, 128), 7.0, device=gpu_device)
    enc = D.DINOImageEncoder(DC.weights("A"))
    _, table, n, cfg = enc._device(gpu_device)
    nbytes = L.gsr_dino_workspace_bytes(C.byref(cfg), 2, 48, 80)
    ws = workspace(nbytes, gpu_device)

    def forward(c=cfg, B=2, H=48, W=80, x0=x, ws_=ws, nb=nbytes, out=pooled, tab=table, nw=n):
        return L.gsr_dino_forward(C.byref(c), tab, nw, ptr(x0), None, B, H, W, ptr(ws_), nb, ptr(out), None, stream(gpu_device))

    def bad(**kw):
        c = good.to_c()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert forward() == 0
    torch.cuda.synchronize()
    pooled.fill_(7.0)
    cases = {"hidden": forward(c=bad(hidden=96)), "heads": forward(c=bad(heads=3)), "intermediate": forward(c=bad(intermediate=500)),
             "H": forward(H=15), "W": forward(W=8), "B0": forward(B=0), "B9": forward(B=9), "ws": forward(nb=nbytes - 1),
             "ws null": forward(ws_=None), "x0": forward(x0=None), "pooled": forward(out=None), "table": forward(nw=n - 1),
             "layers": forward(c=bad(layers=0))}
    assert all(rc == -1 for rc in cases.values()), cases           # GSR_E_INVALID
    for c in (bad(hidden=96), bad(intermediate=500)):
        assert L.gsr_dino_workspace_bytes(C.byref(c), 2, 48, 80) == 0
    assert L.gsr_dino_workspace_bytes(C.byref(cfg), 9, 48, 80) == 0 and L.gsr_dino_workspace_bytes(C.byref(cfg), 1, 15, 80) == 0
    nulls = table.__class__(*table)
    nulls[_lib.GSR_DINO_W_LAYER0 + 2] = None          # q_proj.weight of layer 0
    assert forward(tab=nulls) == -1 and b"weight" in L.gsr_last_error()
    h = torch.zeros(4, 128, dtype=torch.float16, device=gpu_device)
    assert L.gsr_dino_linear(ptr(h), ptr(h), None, None, 4, 100, 4, 0, ptr(h), stream(gpu_device)) == -1        # K % 64
    assert L.gsr_dino_linear(ptr(h), ptr(h), None, None, 4, 128, 4, 2, ptr(h), stream(gpu_device)) == -1        # residual without lambda
    assert L.gsr_dino_linear(ptr(h), ptr(h), None, None, 4, 128, 4, 5, ptr(h), stream(gpu_device)) == -1
    assert L.gsr_dino_attn(ptr(h), None, ptr(h), 1, 4, 2, ptr(h), stream(gpu_device)) == -1
    assert L.gsr_dino_cosine(ptr(h), ptr(h), 0, 1.0, ptr(h), stream(gpu_device)) == -1
    assert L.gsr_dino_rope(ptr(h), ptr(h), 1, 4, 2, 3, 5, 100.0, stream(gpu_device)) == -1                      # Hp Wp > T
    torch.cuda.synchronize()
    assert float(pooled.min()) == 7.0 and float(pooled.max()) == 7.0            # nothing was launched
    with pytest.raises(_lib.GsrError):
        enc.encode_tensor(torch.zeros(3, 48, 80))                               # CPU tensors are refused
    with pytest.raises(_lib.GsrError, match="16x16"):
        enc.encode_tensor(torch.zeros(3, 8, 80, device=gpu_device))


# ---------------------------------------------------------------- train_cli --dino_dir
def _write_scene(root, dev, W=96, H=64):
    from PIL import Image
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.params import PipelineParams
    from gaussmart_amd.scene_io import storePly
    from gaussmart_amd.synthetic import make_scene, jittered_cameras
    os.makedirs(root / "train")
    os.makedirs(root / "test")
    params, _ = make_scene(800, W, H, seed=3, radius_px=5.0)
    cams = jittered_cameras(3, W, H, seed=3, device=dev, amount=0.2)
    m = GaussianModel(3, device=dev)
    m.create_from_params(params)
    frames = {"train": [], "test": []}
    for i, cam in enumerate(cams):
        split = "test" if i == 0 else "train"
        with torch.no_grad():
            img = render(cam, m, PipelineParams(), torch.zeros(3, device=dev), surface_maps=False)["render"].clamp(0, 1)
        rgba = np.concatenate([(img.permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], -1)
        Image.fromarray(rgba, "RGBA").save(root / split / f"r_{i}.png")
        c2w = np.linalg.inv(cam.world_view_transform.T.cpu().numpy().astype(np.float64))
        c2w[:3, 1:3] *= -1
        frames[split].append({"file_path": f"./{split}/r_{i}", "transform_matrix": c2w.tolist()})
    for split in ("train", "test"):
        json.dump({"camera_angle_x": cams[0].FoVx, "frames": frames[split]}, open(root / f"transforms_{split}.json", "w"))
    storePly(str(root / "points3d.ply"), params["xyz"].numpy(), np.full((800, 3), 128))


def test_train_cli_with_dino_dir(gpu_device, tmp_path, monkeypatch):
    from gaussmart_amd import train_cli
    import gaussmart_amd.trainer as T
    root, wdir = tmp_path / "scene", tmp_path / "dino"
    _write_scene(root, gpu_device)
    D.save_dino_weights(DC.weights("A"), wdir)
    seen = []
    real = T.DinoTerm.step

    def spy(self, iteration, cam, image, gt, parts, opt):
        if iteration > self.start_iter:
            seen.append((iteration, image.detach().clone(), gt.detach().clone()))
        return real(self, iteration, cam, image, gt, parts, opt)
    monkeypatch.setattr(T.DinoTerm, "step", spy)
    common = ["-s", str(root), "--iterations", "6", "--save_iterations", "6", "--eval", "--log_every", "0"]
    train_cli.main(common + ["-m", str(tmp_path / "plain")])
    assert not os.path.exists(tmp_path / "plain" / "dino_loss_log.csv")
    dino_args = ["--dino_dir", str(wdir), "--lambda_dino", "0.05", "--dino_start_iter", "2"]
    train_cli.main(common + ["-m", str(tmp_path / "with")] + dino_args)
    kernel_renders, seen[:] = list(seen), []
    train_cli.main(common + ["-m", str(tmp_path / "host")] + dino_args + ["--host"])

    def params(name):
        out = []

        def walk(o):
            if isinstance(o, torch.Tensor):
                out.append(o.detach().cpu())
            elif isinstance(o, dict):
                for k in sorted(o, key=str):
                    walk(o[k])
            elif isinstance(o, (list, tuple)):
                for v in o:
                    walk(v)
        walk(torch.load(tmp_path / name / "chkpnt6.pth", map_location="cpu", weights_only=True)[0])
        return out
    plain, kernels, hosted = params("plain"), params("with"), params("host")
    assert len(plain) > 6 and len(plain) == len(kernels) == len(hosted)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(plain, kernels, hosted))      # no gradient: same trajectory

    def rows(name):
        r = list(csv.reader(open(tmp_path / name / "dino_loss_log.csv")))
        assert r[0] == ["iteration", "dino_loss", "total_loss", "l1_loss", "dist_loss", "normal_loss"]
        return np.array([[float(v) for v in row] for row in r[1:]])
    kern, host = rows("with"), rows("host")
    assert kern[:, 0].tolist() == [1, 2, 3, 4, 5, 6] and (kern[:2, 1] == 0).all() and (kern[2:, 1] != 0).all()
    # the logged values are dino_loss() recomputed from the same render and ground truth
    enc = D.DINOImageEncoder(DC.weights("A"))
    assert [it for it, _, _ in kernel_renders] == [3, 4, 5, 6]
    for (it, image, gt), row in zip(kernel_renders, kern[2:]):
        assert float(dino_loss(image, gt, enc, 0.05)) == row[1], it
    # --host: the whole-model bar on each pooled row carried through the cosine: d cos <= 2 |d a| / |a| + 2 |d b| / |b| in
    # the 2-norm, |d a| <= sqrt(hidden) bar, times lambda, plus the two fp16 roundings of the logged values
    bar = DC.model_bars("A", 64, 96)["pooled"]          # the scene's size
    for (it, image, gt), k, h in zip(kernel_renders, kern[2:], host[2:]):
        emb = enc.encode_pair(image, gt).double().norm(dim=1)
        slack = 0.05 * 2 * (128 ** 0.5) * bar * float((1 / emb).sum()) + 2 * U16 * 0.05
        report(f"train_cli it {it}: kernels {k[1]:.6f}, --host {h[1]:.6f}, bar {slack:.2e}")
        assert abs(k[1] - h[1]) <= slack
    assert np.allclose(kern[:, 2] - kern[:, 1], host[:, 2] - host[:, 1], rtol=0, atol=1e-6)
