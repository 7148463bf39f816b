"""The SAM2 kernels (csrc/sam2.hip; include/gsr.h: HV_EMBED, HV_LINEAR, HV_ATTN, HV_POOL, HV_NECK, and SM_SCORE / SM_EMIT with the
one-step geometry) on the device, everything through the C ABI: each rule against fp64 from the same fp16 inputs with a bar
that follows the roundings the rule states, the whole encoder against transformers' fp64 model with a bar per output map
measured on transformers' own fp16 model, the one-step mask selection against the fp64 torch formulation pixel by pixel
wherever that formulation decides, the generator end to end, the bit-equalities, the refusals, and sam_cli --sam2 feeding
segment_cli.  Cases, twins and the bar arithmetic are in tests/sam2_cases.py.  GSR_SAM2_PARITY_REPORT=<file>: the measured errors
and bars are appended there (profiles/sam2_parity.txt is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sam2_cases as SC
from sam2_cases import U32
from test_gpu_sam import tiny_scan
from gaussmart_amd import _lib
from gaussmart_amd import sam as S1
from gaussmart_amd import sam2 as S2
from gaussmart_amd._dev import ptr, stream, workspace

pytestmark = pytest.mark.gpu


def report(line):
    out = os.environ.get("GSR_SAM2_PARITY_REPORT")
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


# ---------------------------------------------------------------- HV_EMBED
@pytest.mark.parametrize("S_,embed", [(32, 144), (96, 144), (32, 96), (96, 96)])
def test_embed_against_fp64(gpu_device, S_, embed):
    g = torch.Generator().manual_seed(S_ + embed)
    gr = S_ // 4
    x = torch.randn(3, S_, S_, generator=g)
    pw, pb, pos = h16((embed, 3, 7, 7), g, 147 ** -0.5), h16((embed,), g, 0.1), h16((gr, gr, embed), g)
    pw152 = F.pad(pw.reshape(embed, 147), (0, 5)).contiguous()
    L = _lib.lib()
    nbytes = L.gsr_sam2_embed_workspace_bytes(S_)
    ws = workspace(nbytes, gpu_device)
    out = torch.full((gr * gr, embed), float("nan"), device=gpu_device)
    d = [t.to(gpu_device) for t in (x, pw152, pb, pos)]
    _lib.check(L.gsr_sam2_embed(ptr(d[0]), S_, embed, ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(ws), nbytes, ptr(out), stream(gpu_device)))
    x16 = x.to(torch.float16).double()[None]
    u = F.conv2d(x16, pw.double(), pb.double(), stride=4, padding=3)[0].permute(1, 2, 0)         # [g,g,embed]
    mag = F.conv2d(x16.abs(), pw.double().abs(), None, stride=4, padding=3)[0].permute(1, 2, 0)
    want = u + pos.double()
    # the fp32 chain of 152 terms, the bias addition and the position addition (one fp32 rounding each)
    bar = 152 * U32 * mag + U32 * u.abs() + U32 * want.abs() + 2 * U32
    got = out.reshape(gr, gr, embed)
    held(f"embed S{S_} e{embed}", got, want, bar)
    # the border rows and columns on their own: the top and left ones read the padding
    for name, sl in (("top", (0,)), ("left", (slice(None), 0)), ("bottom", (gr - 1,)), ("right", (slice(None), gr - 1))):
        held(f"embed S{S_} e{embed} {name} border", got[sl], want[sl], bar[sl])
    # the padding is zeros and only the top row and the left column read it: ones there move those far beyond the bar, and nothing else
    ones = F.conv2d(F.pad(x16, (3, 3, 3, 3), value=1.0), pw.double(), pb.double(), stride=4)[0].permute(1, 2, 0) + pos.double()
    assert min(float((ones[0] - want[0]).abs().max()), float((ones[:, 0] - want[:, 0]).abs().max())) > 10 * float(bar.max())
    assert torch.allclose(ones[1:, 1:], want[1:, 1:], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- HV_LINEAR
def linear_dev(fn, x, w, b, M, K, N, epi, dev, f32=False):
    out = torch.full((M, N), float("nan"), dtype=torch.float32 if f32 else torch.float16, device=dev)
    d = [t.to(dev) for t in (x, w, b)]
    _lib.check(fn(ptr(d[0]), ptr(d[1]), ptr(d[2]), None, M, K, N, epi, ptr(out), stream(dev)))
    return out


@pytest.mark.parametrize("K", [96, 144, 152, 288])
def test_linear_against_fp64(gpu_device, K):
    M, N = 333, 200                                     # three row blocks and two column blocks, neither a multiple of 128
    g = torch.Generator().manual_seed(K)
    x, w, b = h16((M, K), g), h16((N, K), g, K ** -0.5), h16((N,), g, 0.1)
    L = _lib.lib()
    want = x.double() @ w.double().T + b.double()
    e = (K + 64) * U32 * (x.double().abs() @ w.double().abs().T) + U32 * want.abs()      # the chain (with its zero tail) and the bias addition
    held(f"linear K{K} f32", linear_dev(L.gsr_sam2_linear, x, w, b, M, K, N, _lib.GSR_SAM2_EPI_F32, gpu_device, f32=True), want, e + U32)
    got = linear_dev(L.gsr_sam2_linear, x, w, b, M, K, N, _lib.GSR_DINO_EPI_BIAS, gpu_device)
    held(f"linear K{K} fp16", got, want, e + SC.round16(want, e))
    assert torch.equal(linear_dev(L.gsr_sam2_linear, x, w, b, M, K, N, _lib.GSR_DINO_EPI_BIAS, gpu_device), got)
    # a K that is no multiple of 8 is refused
    assert L.gsr_sam2_linear(ptr(got), ptr(got), None, None, M, K + 4, N, 0, ptr(got), stream(gpu_device)) == -1


def test_linear_bits_equal_dino_linear_at_k128(gpu_device):
    M, K, N = 333, 128, 200
    g = torch.Generator().manual_seed(128)
    x, w, b = h16((M, K), g), h16((N, K), g, K ** -0.5), h16((N,), g, 0.1)
    L = _lib.lib()
    for epi in (_lib.GSR_DINO_EPI_BIAS, _lib.GSR_DINO_EPI_GELU):
        a = linear_dev(L.gsr_sam2_linear, x, w, b, M, K, N, epi, gpu_device)
        assert torch.equal(a, linear_dev(L.gsr_dino_linear, x, w, b, M, K, N, epi, gpu_device)) and torch.isfinite(a).all()
    # gsr_dino_linear keeps its own checks
    assert L.gsr_dino_linear(ptr(a), ptr(a), None, None, M, 96, N, 0, ptr(a), stream(gpu_device)) == -1


# ---------------------------------------------------------------- HV_ATTN
def attn_dev(qkv, g, w, stride, heads, hd, dev):
    go = g // stride
    out = torch.full((go * go, heads * hd), float("nan"), dtype=torch.float16, device=dev)
    d = qkv.to(dev)
    _lib.check(_lib.lib().gsr_sam2_attn(ptr(d), g, w, stride, heads, hd, ptr(out), stream(dev)))
    return out


ATTN_SHAPES = [(16, 8, 1, 2, 72), (16, 4, 1, 1, 96), (16, 16, 1, 2, 72), (16, 0, 1, 4, 72), (32, 0, 1, 2, 96),
               (16, 8, 2, 2, 72), (16, 4, 2, 2, 96), (32, 16, 2, 4, 72), (16, 8, 1, 2, 56), (16, 4, 2, 1, 64), (16, 8, 1, 2, 80)]


@pytest.mark.parametrize("g,w,stride,heads,hd", ATTN_SHAPES)
def test_attention_against_fp64(gpu_device, g, w, stride, heads, hd):
    gen = torch.Generator().manual_seed(1000 * g + 10 * w + stride + hd)
    qkv = h16((g * g, 3 * heads * hd), gen)
    want, bar = SC.attention64(qkv, g, w, stride, heads, hd)
    got = attn_dev(qkv, g, w, stride, heads, hd, gpu_device)
    held(f"attn g{g} w{w} stride{stride} heads{heads} hd{hd}", got, want, bar)
    assert torch.equal(attn_dev(qkv, g, w, stride, heads, hd, gpu_device), got)          # the same bits again
    if stride == 2:
        # the pooling is a maximum: the mean of the four rows moves the output far beyond the bar
        s, hidden = w, heads * hd
        avg = qkv.clone().reshape(g // 2, 2, g // 2, 2, 3 * hidden)
        avg[..., :hidden] = avg[..., :hidden].float().mean((1, 3), keepdim=True).to(torch.float16)
        assert float((SC.attention64(avg.reshape(g * g, -1), g, w, 2, heads, hd)[0] - want).abs().max()) > 10 * float(bar.max())
    if w and w < g:
        # a window's output depends on its own tokens only: new tokens in window (0, 1) leave every other window's bits alone
        other = qkv.clone().reshape(g, g, -1)
        other[:w, w:2 * w] = h16((w, w, other.shape[-1]), gen)
        moved = attn_dev(other.reshape(g * g, -1), g, w, stride, heads, hd, gpu_device)
        so, go = w // stride, g // stride
        same = torch.ones(go, go, dtype=torch.bool)
        same[:so, so:2 * so] = False
        a, b = got.reshape(go, go, -1).cpu(), moved.reshape(go, go, -1).cpu()
        assert torch.equal(a[same], b[same]) and not torch.equal(a[~same], b[~same])


# ---------------------------------------------------------------- HV_POOL
@pytest.mark.parametrize("g,Cn", [(6, 37), (64, 288)])
def test_pool_is_exact(gpu_device, g, Cn):
    x = torch.randn(g, g, Cn, generator=torch.Generator().manual_seed(g))
    x[1, 1] = -0.0
    out = torch.full((g // 2, g // 2, Cn), float("nan"), device=gpu_device)
    d = x.to(gpu_device)
    _lib.check(_lib.lib().gsr_sam2_pool(ptr(d), g, Cn, ptr(out), stream(gpu_device)))
    assert torch.equal(out.cpu(), F.max_pool2d(x.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))


# ---------------------------------------------------------------- HV_NECK
def test_neck_against_fp64(gpu_device):
    g0, embed, D = 64, 144, 256                         # H1's four grids and widths
    gen = torch.Generator().manual_seed(64)
    dims, grids = [embed << i for i in range(4)], [g0 >> i for i in range(4)]
    xs = [2.0 * torch.randn(grids[i] ** 2, dims[i], generator=gen) for i in range(4)]
    lw = [h16((D, dims[i]), gen, dims[i] ** -0.5) for i in range(4)]
    lb = [h16((D,), gen, 0.1) for i in range(4)]
    s0w, s0b, s1w, s1b = h16((D // 8, D), gen, D ** -0.5), h16((D // 8,), gen, 0.1), h16((D // 4, D), gen, D ** -0.5), h16((D // 4,), gen, 0.1)
    nomem = torch.randn(D, generator=gen)
    weights = [t for i in range(4) for t in (lw[i], lb[i])] + [s0w, s0b, s1w, s1b, nomem]

    def run(weights, mask=0b1100):
        L = _lib.lib()
        nbytes = L.gsr_sam2_neck_workspace_bytes(g0, embed, D)
        ws = workspace(nbytes, gpu_device)
        dx, dw = [t.to(gpu_device) for t in xs], [t.to(gpu_device) for t in weights]
        outs = [torch.full((c, gi, gi), float("nan"), device=gpu_device) for c, gi in ((D // 8, grids[0]), (D // 4, grids[1]), (D, grids[2]))]
        streams = (C.c_void_p * 4)(*[t.data_ptr() for t in dx])
        table = (C.c_void_p * 13)(*[t.data_ptr() for t in dw])
        _lib.check(L.gsr_sam2_neck(streams, g0, embed, D, mask, table, ptr(ws), nbytes, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream(gpu_device)))
        return [o.cpu() for o in outs]

    # fp64 from the same fp16 inputs: the streams rounded to fp16 are part of the rule
    lat, elat = [], []
    for i in range(4):
        x16 = xs[i].to(torch.float16).double()
        v = x16 @ lw[i].double().T + lb[i].double()
        lat.append(v)
        elat.append((dims[i] + 64) * U32 * (x16.abs() @ lw[i].double().abs().T) + U32 * v.abs())

    def up(t, g):       # [g/2 g/2,D] -> [g g,D], nearest
        return t.reshape(g // 2, g // 2, D).repeat_interleave(2, 0).repeat_interleave(2, 1).reshape(g * g, D)
    prev2 = lat[2] + up(lat[3], grids[2])
    e2 = elat[2] + up(elat[3], grids[2]) + U32 * prev2.abs()
    want2 = prev2 + nomem.double()
    got = run(weights)
    held("neck level 2", got[2].reshape(D, -1).T, want2, e2 + U32 * want2.abs() + U32)
    for i, (sw, sb) in enumerate(((s0w, s0b), (s1w, s1b))):
        ph = lat[i]                                 # levels 0 and 1 are the lateral alone under the default [2, 3]
        eph = elat[i] + SC.round16(ph, elat[i])
        want = ph @ sw.double().T + sb.double()
        bar = eph @ sw.double().abs().T + (D + 64) * U32 * ((ph.abs() + eph) @ sw.double().abs().T) + U32 * want.abs() + U32
        held(f"neck level {i}", got[i].reshape(sw.shape[0], -1).T, want, bar)
    # what must be caught: a zeroed no_memory_embedding, a dropped top-down path, conv_s0 and conv_s1 exchanged
    bar2 = float((e2 + U32 * want2.abs() + U32).max())
    assert float((prev2 - want2).abs().max()) > 10 * bar2 and float((lat[2] + nomem.double() - want2).abs().max()) > 10 * bar2
    zero = run(weights[:12] + [torch.zeros(D)])
    assert float((zero[2].reshape(D, -1).T.double() - prev2).abs().max()) <= bar2
    flat = run(weights, mask=0)
    assert float((flat[2].reshape(D, -1).T.double() - (lat[2] + nomem.double())).abs().max()) <= bar2
    assert float(((lat[0] @ s1w.double()[:D // 8].T + s1b.double()[:D // 8]) - (lat[0] @ s0w.double().T + s0b.double())).abs().max()) > 10 * float(bar.max())
    # every level that is marked receives the level above: with all bits set level 0 carries levels 1, 2 and 3
    full = run(weights, mask=0b1111)
    p1 = lat[1] + up(prev2, grids[1])
    p0 = lat[0] + up(p1, grids[0])
    want0 = p0 @ s0w.double().T + s0b.double()
    assert float((full[0].reshape(D // 8, -1).T.double() - want0).abs().max()) < 0.05 < float((want0 - (lat[0] @ s0w.double().T + s0b.double())).abs().max())


# ---------------------------------------------------------------- the whole encoder
@pytest.fixture(scope="module")
def encoders():
    return {}


def encode(name, dev, encoders):
    if name not in encoders:
        encoders[name] = S2.Sam2ImageEncoder(SC.weights(name))
    return encoders[name].encode(SC.pixels(name).to(dev))


@pytest.mark.parametrize("name", ["H1", "H2"])
def test_encoder_against_the_twin(gpu_device, name, encoders):
    bars = SC.model_bars(name)
    report(SC.bars_line(name, bars))
    got = encode(name, gpu_device, encoders)
    assert [tuple(m.shape) for m in got] == [(32, 64, 64), (64, 32, 32), (256, 16, 16)] and all(m.dtype == torch.float32 for m in got)
    for k in range(3):
        held(f"encoder {name} map {k}", got[k], SC.twin(name)[k], bars[k]["bar"])
    again = encode(name, gpu_device, encoders)
    assert all(torch.equal(a, b) for a, b in zip(again, got))            # the same bits on every run


# ---------------------------------------------------------------- SM_SCORE / SM_EMIT, one step
def score_dev(logits, mask_size, dev, skip=None, tau=0.0, delta=1.0):
    n, Lr = logits.shape[0], logits.shape[-1]
    counts = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
    boxes = torch.full((n, 4), -7.0, device=dev)
    _lib.check(_lib.lib().gsr_sam_mask_score_direct(ptr(logits), n, Lr, *mask_size, tau, delta, ptr(skip), ptr(counts), ptr(boxes), stream(dev)))
    return counts, boxes


def emit_dev(logits, mask_size, index, dev, tau=0.0):
    n, Lr, m = logits.shape[0], logits.shape[-1], len(index)
    out = torch.full((m, *mask_size), 9, dtype=torch.uint8, device=dev)
    idx = torch.as_tensor(index, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().gsr_sam_mask_emit_direct(ptr(logits), n, Lr, *mask_size, tau, ptr(idx), m, ptr(out), stream(dev)))
    return out


@pytest.mark.parametrize("Lr,cone_size,mask_size,n", SC.MASK_SHAPES)
def test_one_step_score_and_emit_against_fp64(gpu_device, Lr, cone_size, mask_size, n):
    logits = SC.mask_logits(Lr, *cone_size, n=n)
    truth = SC.mask_truth(logits, mask_size)
    dl = logits.to(gpu_device)
    counts, boxes = score_dev(dl, mask_size, gpu_device)
    planes = emit_dev(dl, mask_size, list(range(n)), gpu_device)
    again = score_dev(dl, mask_size, gpu_device)
    assert torch.equal(again[0], counts) and torch.equal(again[1], boxes)
    assert torch.equal(planes.flatten(1).sum(1, dtype=torch.int32), counts[:, 0]) and int(planes.max()) <= 1
    planes, counts, boxes = planes.cpu().bool(), counts.cpu().long(), boxes.cpu()
    on, decided = truth["on"], truth["decided"]
    und = (~decided).flatten(1).sum(1)
    share = float(und.sum()) / decided.numel()
    flips = int(((planes != on) & decided).sum())
    worst = int(((counts - truth["counts"]).abs().max(1).values - und).max())
    report(f"one-step masks L{Lr} -> {mask_size} n{n}: undecided share {share:.2e}, decided pixels that differ {flips}, "
           f"worst count difference minus undecided {worst}")
    assert share <= 1e-3
    assert flips == 0                                              # every decided pixel agrees exactly
    assert worst <= 0                                              # counts differ by at most the mask's undecided pixels
    H, W = mask_size
    ys, xs = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    checked = 0
    for k in range(n):
        sure = on[k] & decided[k]
        if not sure.any():
            if und[k] == 0:
                assert boxes[k].tolist() == [0, 0, 0, 0] and counts[k, 0] == 0
                checked += 1
            continue
        box = [int(xs[sure].min()), int(ys[sure].min()), int(xs[sure].max()), int(ys[sure].max())]
        loose = ~decided[k]
        outside = loose & ((xs < box[0]) | (xs > box[2]) | (ys < box[1]) | (ys > box[3]))
        if not outside.any():
            assert boxes[k].tolist() == box, (k, boxes[k].tolist(), box)
            checked += 1
    report(f"one-step masks L{Lr} -> {mask_size} n{n}: {checked} boxes had no undecided pixel outside them and were compared exactly")
    assert checked >= 2                                            # the constant masks at the least
    assert counts[0].tolist() == [0, 0, 0] and boxes[0].tolist() == [0, 0, 0, 0]
    assert counts[1].tolist() == [H * W] * 3 and boxes[1].tolist() == [0, 0, W - 1, H - 1]
    # a skipped mask is not read and reports zeros; SM_EMIT of a list; an index outside the masks is a zero plane
    skip = torch.zeros(n, dtype=torch.uint8, device=gpu_device)
    skip[3] = 1
    poisoned = dl.clone()
    poisoned[3] = float("nan")
    c2, b2 = score_dev(poisoned, mask_size, gpu_device, skip)
    keep = torch.arange(n) != 3
    assert c2[3].tolist() == [0, 0, 0] and torch.equal(c2.cpu().long()[keep], counts[keep]) and torch.equal(b2.cpu()[keep], boxes[keep])
    some = emit_dev(dl, mask_size, [5, 1, n, 2], gpu_device).cpu().bool()
    assert torch.equal(some[0], planes[5]) and torch.equal(some[1], planes[1]) and not some[2].any() and torch.equal(some[3], planes[2])


# ---------------------------------------------------------------- the generator end to end
def test_generator_end_to_end(gpu_device, tmp_path):
    from PIL import Image
    tiny_scan(str(tmp_path / "scan"))
    image = np.asarray(Image.open(str(tmp_path / "scan" / "images" / "0000.png")).convert("RGB"))
    w = SC.weights("H1")
    gen = S2.Sam2MaskGenerator(w, points_per_side=8, device=gpu_device)
    e = gen.embed(image)
    assert [tuple(m.shape) for m in e["emb"]] == [(32, 64, 64), (64, 32, 32), (256, 16, 16)]
    assert e["input_size"] == (256, 256) and e["mask_size"] == (96, 128)
    points = S1.point_grid(8, e["input_size"])
    low, iou = gen.decode(e["emb"], points)
    assert low.shape == (64, 3, 64, 64) and iou.shape == (64, 3) and torch.isfinite(low).all()
    # thresholds: the medians of this run's own iou and fp64 stability scores
    truth = SC.mask_truth(low.reshape(-1, 64, 64).cpu(), e["mask_size"])
    s64 = truth["counts"][:, 1].double() / truth["counts"][:, 2].double()
    gen.pred_iou_thresh = float(iou.median())
    gen.stability_score_thresh = float(s64[~torch.isnan(s64)].median())
    sel = gen.select(low, iou, e["input_size"], e["mask_size"])
    host = S1.select_host(low, iou, e["input_size"], e["mask_size"], gen.pred_iou_thresh, gen.stability_score_thresh,
                          gen.stability_score_offset, gen.box_nms_thresh, dtype=torch.float64, direct=True)
    und = (~truth["decided"]).flatten(1).sum(1)
    inter, union = truth["counts"][:, 1].double(), truth["counts"][:, 2].double()
    lo, hi = (inter - und).clamp(min=0) / (union + und), (inter + und) / (union - und).clamp(min=1)
    firm = ((lo >= gen.stability_score_thresh) | (hi < gen.stability_score_thresh) | (union == 0)).to(gpu_device)
    report(f"sam2 generator: {int(sel['keep_in'].sum())} of {len(firm)} candidates pass both gates, {len(sel['index'])} masks after NMS, "
           f"{int((~firm).sum())} candidates undecided")
    assert torch.equal(sel["keep_in"][firm], host["keep_in"][firm]) and 0 < len(sel["index"]) < 192
    if bool(firm.all()) and int(und.sum()) == 0:
        assert torch.equal(sel["index"], host["index"]) and torch.equal(sel["masks"], host["masks"])
        assert torch.equal(sel["boxes"], host["boxes"]) and torch.equal(sel["area"], host["area"])
    # the reference's list of dicts, with an NMS threshold no IoU exceeds (see tests/test_gpu_sam.py)
    gen2 = S2.Sam2MaskGenerator(w, points_per_side=8, pred_iou_thresh=gen.pred_iou_thresh,
                                stability_score_thresh=gen.stability_score_thresh, box_nms_thresh=1.0, device=gpu_device)
    masks = gen2.generate(image)
    assert len(masks) == int(sel["keep_in"].sum()) > 8 and set(gen2.last_ms) == {"embed", "decode", "select"}
    piou = [m["predicted_iou"] for m in masks]
    assert piou == sorted(piou, reverse=True) and piou[0] == float(sel["predicted_iou"][0])
    for m in masks:
        seg = m["segmentation"]
        assert set(m) == {"segmentation", "area", "bbox", "predicted_iou", "point_coords", "stability_score", "crop_box"}
        assert seg.shape == (96, 128) and seg.dtype == bool and m["area"] == int(seg.sum()) > 0
        ys, xs = np.nonzero(seg)
        x, y, bw, bh = m["bbox"]
        assert (x, y, x + bw, y + bh) == (xs.min(), ys.min(), xs.max(), ys.max())
        # the gate compares in fp32 (the threshold here IS one candidate's fp64 score, the median)
        assert m["crop_box"] == [0, 0, 128, 96] and np.float32(m["stability_score"]) >= np.float32(gen.stability_score_thresh)
        assert m["predicted_iou"] > gen.pred_iou_thresh and len(m["point_coords"]) == 1
        px, py = m["point_coords"][0]
        assert 0 < px < 128 and 0 < py < 96                        # the grid point in the picture's own frame
    dev_masks = gen2.generate_device(image)
    assert dev_masks.is_cuda and dev_masks.dtype == torch.uint8 and np.array_equal(dev_masks.cpu().numpy().astype(bool), np.array([m["segmentation"] for m in masks]))


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(gpu_device):
    L = _lib.lib()
    cfg = SC.config("H2")
    tensors = SC.weights("H2").to(gpu_device).table()
    x = SC.pixels("H2").to(gpu_device)
    i4 = C.c_int32 * 4

    def make(image=256, windows=(8, 4, 16, 8), stride=(2, 2), dims=None, heads=None, glob=(3,), eps=1e-6):
        keep = (C.c_int32 * len(glob))(*glob)
        return _lib.GsrSam2Config(image, 256, 0b1100, len(glob), i4(*cfg.blocks_per_stage), i4(*(dims or cfg.dims())), i4(*(heads or cfg.heads())),
                                  i4(*windows), (C.c_int32 * 2)(*stride), eps, keep), keep

    good, keep_good = make()
    nbytes = L.gsr_sam2_workspace_bytes(C.byref(good))
    assert nbytes > 0
    ws = workspace(nbytes, gpu_device)

    def call(short=0, null=None, n=None, **kw):
        c, keep = make(**kw)
        table = (C.c_void_p * len(tensors))(*[None if (t is None or i == null) else t.data_ptr() for i, t in enumerate(tensors)])
        outs = [torch.full(s, -3.0, device=gpu_device) for s in ((32, 64, 64), (64, 32, 32), (256, 16, 16))]
        rc = L.gsr_sam2_encode(C.byref(c), table, len(tensors) if n is None else n, ptr(x), ptr(ws), nbytes - short, ptr(outs[0]), ptr(outs[1]),
                               ptr(outs[2]), stream(gpu_device))
        torch.cuda.synchronize(gpu_device)
        return rc, all(bool((o == -3.0).all()) for o in outs), L.gsr_sam2_workspace_bytes(C.byref(c))

    assert call()[:2] == (0, False)
    for kw in (dict(windows=(8, 4, 14, 8)),             # a stage grid that is no multiple of its window
               dict(image=128),                         # stock windows: S % 256 != 0
               dict(stride=(1, 1)), dict(stride=(2, 1)),
               dict(dims=(96, 192, 384, 700)),          # a stage that does not double its width
               dict(glob=(2,)),                         # a global block that starts a stage (block 2 is the first of stage 2)
               dict(heads=(2, 4, 8, 16)),               # head_dim 48
               dict(eps=1e-5),
               dict(short=256), dict(null=0), dict(null=5), dict(null=len(tensors) - 1), dict(n=len(tensors) - 1)):
        rc, untouched, nb = call(**kw)
        assert rc == -1 and untouched, kw                               # GSR_E_INVALID, and the outputs are still at their fill value
        assert len(L.gsr_last_error()) > 10
        if not {"short", "null", "n"} & set(kw):
            assert nb == 0, kw
    # the stage entry points
    q = torch.zeros(256, 3 * 144, dtype=torch.float16, device=gpu_device)
    o = torch.full((256, 144), -3.0, dtype=torch.float16, device=gpu_device)
    of = torch.full((256, 144), -3.0, device=gpu_device)
    st = stream(gpu_device)
    for g, w, stride, heads, hd in ((16, 8, 1, 3, 48), (16, 5, 1, 2, 72), (16, 8, 3, 2, 72), (16, 0, 2, 2, 72), (16, 3, 2, 2, 72), (16, 32, 1, 2, 72)):
        assert L.gsr_sam2_attn(ptr(q), g, w, stride, heads, hd, ptr(o), st) == -1
    assert L.gsr_sam2_attn(None, 16, 8, 1, 2, 72, ptr(o), st) == -1
    assert L.gsr_sam2_linear(ptr(q), ptr(q), None, None, 16, 100, 16, 0, ptr(o), st) == -1             # K no multiple of 8
    assert L.gsr_sam2_linear(ptr(q), ptr(q), None, None, 16, 96, 16, 3, ptr(o), st) == -1              # the DINO embedding's scatter
    assert L.gsr_sam2_linear(ptr(q), ptr(q), None, None, 16, 96, 16, _lib.GSR_DINO_EPI_RESID, ptr(of), st) == -1      # no lambda
    assert L.gsr_sam2_pool(ptr(of), 15, 8, ptr(of), st) == -1
    assert L.gsr_sam2_embed(ptr(of), 30, 144, ptr(q), ptr(q), ptr(q), ptr(ws), nbytes, ptr(of), st) == -1
    assert L.gsr_sam2_embed(ptr(of), 32, 144, ptr(q), ptr(q), ptr(q), ptr(ws), 64, ptr(of), st) == -1
    assert L.gsr_sam2_neck_workspace_bytes(60, 144, 256) == 0 and L.gsr_sam2_neck_workspace_bytes(64, 144, 100) == 0
    assert L.gsr_sam_mask_score_direct(ptr(of), 1, 0, 10, 10, 0.0, 1.0, None, ptr(q), ptr(of), st) == -1
    assert L.gsr_sam_mask_emit_direct(ptr(of), 1, 16, 10, 0, 0.0, ptr(q), 1, ptr(q), st) == -1
    torch.cuda.synchronize(gpu_device)
    assert bool((o == -3.0).all()) and bool((of == -3.0).all())
    with pytest.raises(_lib.GsrError):
        S2.Sam2ImageEncoder(SC.weights("H2")).encode(SC.pixels("H2"))          # a host tensor


# ---------------------------------------------------------------- sam_cli --sam2 -> segment_cli
def test_sam_cli_sam2_feeds_segment_cli(gpu_device, tmp_path, capsys):
    from gaussmart_amd import sam_cli, segment_cli
    scan, out, ckpt = str(tmp_path / "scan"), str(tmp_path / "out"), str(tmp_path / "ckpt")
    tiny_scan(scan)
    S2.save_sam2_weights(SC.weights("H1"), ckpt)
    # random weights predict no iou near 0.86: the gates are opened so that the files hold masks
    sam_cli.main(["--sam2", "-s", scan, "-o", out, "--views", "1", "0", "--sam_checkpoint", ckpt, "--points_per_side", "4", "--device", str(gpu_device),
                  "--pred_iou_thresh", "-100", "--stability_score_thresh", "0.0"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["view"] for l in lines] == [1, 0] and all({"masks", "embed_ms", "decode_ms", "select_ms"} <= set(l) for l in lines)
    assert sorted(os.listdir(os.path.join(out, "segments", "images"))) == ["0000.png", "0001.png"]
    for k in range(2):
        with np.load(os.path.join(out, "segments", "masks", f"segments_{k:03d}.npz")) as z:
            assert set(z.files) == {"masks", "boxes", "areas"} and z["masks"].shape[1:] == (96, 128) and len(z["masks"]) == lines[k]["masks"]
    assert all(l["masks"] > 0 for l in lines)
    with pytest.raises(SystemExit):
        sam_cli.main(["--sam2", "--model_type", "vit_h", "-s", scan, "-o", out, "--views", "0", "--sam_checkpoint", ckpt])
    capsys.readouterr()
    segment_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--masks", os.path.join(out, "segments", "masks"), "--views", "1", "0"])
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert info["points"] == 200 and os.path.exists(os.path.join(out, "segments", "point_cloud", "segment_indices.npy"))
