"""The SAM decoder kernels (csrc/sam_decoder.hip; include/gsr.h: SD_PROMPT, SD_IMAGE, SD_TOKENS, SD_T2I, SD_I2T, SD_UP,
SD_HEADS) on the device, everything through the C ABI: the prompt encoding and the three image-side stages against fp64
restatements of their rules with bars built from the stated roundings (and one named wrong reading each that must exceed
them tenfold), the whole decoder against transformers' fp64 modules with a bar measured on transformers' own fp16 modules,
the bit-equalities, the generator and sam_cli with decoder="hip", and the refusals.  Cases, twins and bars are in
tests/sam_decoder_cases.py.  GSR_SAM_DECODER_PARITY_REPORT=<file>: the measured errors and bars are appended there
(profiles/sam_decoder_parity.txt is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sam_decoder_cases as DC
from gaussmart_amd import _lib
from gaussmart_amd import sam as S
from gaussmart_amd._dev import ptr, stream, workspace

pytestmark = pytest.mark.gpu


def report(line):
    out = os.environ.get("GSR_SAM_DECODER_PARITY_REPORT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


def held(name, got, want64, bar):
    """max over the elements of |got - want| / bar must be <= 1; the figure is reported before it is asserted."""
    err = (got.detach().double().cpu() - want64).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64)
    use = float((err / bar).max())
    report(f"{name}: max err {float(err.max()):.3e}, max bar {float(bar.max()):.3e}, worst err/bar {use:.3f}")
    assert torch.isfinite(got).all() and use <= 1.0, (name, use)


def moved(name, wrong64, want64, bar):
    """a wrong reading must move the fp64 result by more than 10 x the largest bar"""
    bar = torch.as_tensor(bar, dtype=torch.float64)
    d = float((wrong64 - want64).abs().max())
    report(f"{name}: moves the result by {d:.3e} = {d / float(bar.max()):.1f} x the largest bar")
    assert d > 10 * float(bar.max()), name


# ---------------------------------------------------------------- SD_PROMPT
def test_prompt_against_fp64(gpu_device):
    w = DC.weights("D1")
    S_ = w.config.image_size
    pts = torch.cat([DC.points("D1"), torch.tensor([[0.0, 0.0], [S_ - 1.0, S_ - 9.0], [37.3125, 61.71875]])])
    G = w.tensors["prompt_encoder.shared_embedding.positional_embedding"]
    p1, nap = (w.tensors[f"prompt_encoder.{k}.weight"].to(torch.float16) for k in ("point_embed.1", "not_a_point_embed"))
    out = torch.full((len(pts), 2, 256), -3.0, device=gpu_device)
    d = [t.to(gpu_device).contiguous() for t in (pts, G, p1, nap)]
    _lib.check(_lib.lib().gsr_sam_dec_prompt(ptr(d[0]), len(pts), S_, ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(out), stream(gpu_device)))
    want, bar = DC.prompt64(pts, S_, G, p1, nap)
    held("prompt", out, want, bar)
    assert torch.equal(out[:, 1].cpu(), nap.float().reshape(1, 256).expand(len(pts), 256))
    moved("prompt, the padding point encoded instead of not_a_point_embed", DC.prompt64(pts, S_, G, p1, nap, True)[0], want, bar)
    # against the module itself (fp32): the same tokens within the same bar
    prompt = S.host_decoder(w, torch.float64, "cpu")[0]
    with torch.no_grad():
        sparse = prompt(pts.double()[None, :, None, :], torch.ones(1, len(pts), 1, dtype=torch.int64), None, None)[0][0]
    # the module holds fp32 point_embed / not_a_point; the table rounds them to fp16 (random weights are fp16 already)
    held("prompt against SamPromptEncoder fp64", out, sparse, bar)


# ---------------------------------------------------------------- SD_T2I
def t2i_dev(q, kx, kpe, v, P, T, shared, dev):
    out = torch.full((P, 7, 128), -3.0, dtype=torch.float16, device=dev)
    d = [None if t is None else t.to(dev).contiguous() for t in (q, kx, kpe, v)]
    _lib.check(_lib.lib().gsr_sam_dec_t2i(ptr(d[0]), ptr(d[1]), None if kpe is None else ptr(d[2]), ptr(d[3]), P, T, int(shared), ptr(out),
                                          stream(dev)))
    return out


@pytest.mark.parametrize("g,P", [(7, 1), (9, 5), (17, 67)])
def test_t2i_against_fp64(gpu_device, g, P):
    T = g * g
    gen = torch.Generator().manual_seed(100 * g + P)
    q = 2.0 * torch.randn(P, 7, 128, generator=gen)
    kpe = torch.randn(T, 128, generator=gen)
    for shared in (False, True):
        shape = (T, 128) if shared else (P, T, 128)
        kx, v = DC.h16(shape, gen), DC.h16(shape, gen)
        got = t2i_dev(q, kx, kpe, v, P, T, shared, gpu_device)
        want, bar = DC.t2i64(q, kx, kpe, v, shared)
        held(f"t2i g{g} P{P} shared{int(shared)}", got, want, bar)
        if not shared:
            moved(f"t2i g{g} P{P}: scale 32^-1/2", DC.t2i64(q, kx, kpe, v, shared, scale=32 ** -0.5)[0], want, bar)
            moved(f"t2i g{g} P{P}: keys without the positional term", DC.t2i64(q, kx, None, v, shared)[0], want, bar)
            none = t2i_dev(q, kx, None, v, P, T, shared, gpu_device)
            held(f"t2i g{g} P{P} no kpe", none, *DC.t2i64(q, kx, None, v, shared))
            # a point's bits do not depend on the others
            k = P - 1
            alone = t2i_dev(q[k:k + 1], kx[k:k + 1], kpe, v[k:k + 1], 1, T, False, gpu_device)
            assert torch.equal(alone[0], got[k])


# ---------------------------------------------------------------- SD_I2T
@pytest.mark.parametrize("g,P", [(7, 1), (9, 5), (17, 67)])
def test_i2t_against_fp64(gpu_device, g, P):
    T, L = g * g, _lib.lib()
    gen = torch.Generator().manual_seed(200 * g + P)
    qpe, k, v = torch.randn(T, 128, generator=gen), 2.0 * torch.randn(P, 7, 128, generator=gen), torch.randn(P, 7, 128, generator=gen)
    ow, ob = DC.h16((256, 128), gen, 128 ** -0.5), DC.h16((256,), gen, 0.1)
    lw, lb = (0.5 + torch.rand(256, generator=gen)).to(torch.float16), DC.h16((256,), gen, 0.1)
    nbytes = L.gsr_sam_dec_i2t_workspace_bytes(P, T)
    assert nbytes > 0
    ws = workspace(nbytes, gpu_device)
    for shared in (False, True):
        qx = DC.h16((T, 128) if shared else (P, T, 128), gen)
        x = DC.h16((T, 256) if shared else (P, T, 256), gen)
        out = torch.full((P, T, 256), -3.0, dtype=torch.float16, device=gpu_device)
        d = [t.to(gpu_device).contiguous() for t in (qx, qpe, k, v, x, ow, ob, lw, lb)]
        _lib.check(L.gsr_sam_dec_i2t(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), P, T, int(shared), ptr(d[5]), ptr(d[6]), ptr(d[7]),
                                     ptr(d[8]), ptr(ws), nbytes, ptr(out), stream(gpu_device)))
        want, bar = DC.i2t64(qx, qpe, k, v, x, shared, ow, ob, lw, lb)
        held(f"i2t g{g} P{P} shared{int(shared)}", out, want, bar)
        if not shared:
            moved(f"i2t g{g} P{P}: layer_norm4 left out", DC.i2t64(qx, qpe, k, v, x, shared, ow, ob, lw, lb, norm=False)[0], want, bar)
            # in place, and alone: the same bits
            _lib.check(L.gsr_sam_dec_i2t(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), P, T, 0, ptr(d[5]), ptr(d[6]), ptr(d[7]),
                                         ptr(d[8]), ptr(ws), nbytes, ptr(d[4]), stream(gpu_device)))
            assert torch.equal(d[4], out)


# ---------------------------------------------------------------- SD_UP
@pytest.mark.parametrize("g", [7, 9])
def test_upscale_against_fp64(gpu_device, g):
    P, T, L = 5, g * g, _lib.lib()
    w = DC.weights("D1")
    table = w.decoder_table()
    up = _lib.GSR_SAMD_W_UP
    gen = torch.Generator().manual_seed(300 + g)
    x = DC.h16((P, T, 256), gen)
    hyper4 = torch.randn(P, 4, 32, generator=gen)                      # the four mask tokens' rows; the kernels get 1..3
    hyper = hyper4[:, 1:].permute(1, 0, 2).contiguous()                # [3,P,32]
    nbytes = L.gsr_sam_dec_upscale_workspace_bytes(g, P)
    assert nbytes > 0
    ws = workspace(nbytes, gpu_device)
    out = torch.full((P, 3, 4 * g, 4 * g), -3.0, device=gpu_device)
    d = [t.to(gpu_device).contiguous() for t in [x] + table[up:up + 6] + [hyper]]
    _lib.check(L.gsr_sam_dec_upscale(ptr(d[0]), g, P, *[ptr(t) for t in d[1:7]], ptr(d[7]), ptr(ws), nbytes, ptr(out), stream(gpu_device)))
    md = "mask_decoder."
    mod = [w.tensors[md + k].to(torch.float16) for k in S.DEC_UP]
    want, bar = DC.up64(x, g, *mod, hyper4[:, 1:])
    held(f"upscale g{g}", out, want, bar)
    moved(f"upscale g{g}: conv1's taps transposed", DC.up64(x, g, *mod, hyper4[:, 1:], swap1=True)[0], want, bar)
    moved(f"upscale g{g}: conv2's taps transposed", DC.up64(x, g, *mod, hyper4[:, 1:], swap2=True)[0], want, bar)
    moved(f"upscale g{g}: mask tokens 0..2", DC.up64(x, g, *mod, hyper4[:, :3])[0], want, bar)


# ---------------------------------------------------------------- the whole decoder
def decode_dev(name, dev, pts=None, table=None, n=None, g=None, short=0, fill=None):
    """(rc, low_res, iou) of gsr_sam_decode on case `name`."""
    L = _lib.lib()
    w = DC.weights(name)
    g = w.config.grid if g is None else g
    gen = S.SamMaskGenerator(w, device=dev, decoder="hip")
    h = gen._decoder_hip()
    pts = DC.points(name) if pts is None else pts
    P = len(pts)
    emb = DC.embedding(name).reshape(256, w.config.grid, w.config.grid).to(dev).contiguous()
    p = pts.to(dev).contiguous()
    nbytes = max(L.gsr_sam_decode_workspace_bytes(w.config.grid, max(P, 1)), 256)
    ws = workspace(nbytes, dev)
    gg = w.config.grid
    low = torch.full((max(P, 1), 3, 4 * gg, 4 * gg), -3.0 if fill is None else fill, device=dev)
    iou = torch.full((max(P, 1), 3), -3.0 if fill is None else fill, device=dev)
    rc = L.gsr_sam_decode(g, h["table"] if table is None else table, h["n"] if n is None else n, ptr(emb), ptr(h["wide"]), ptr(p), P,
                          16 * g, ptr(ws), nbytes - short, ptr(low), ptr(iou), stream(dev))
    torch.cuda.synchronize(dev)
    return rc, low, iou, h


@pytest.mark.parametrize("name", ["D1", "D2", "D3"])
def test_decoder_against_the_twin(gpu_device, name):
    b = DC.model_bars(name)
    DC.check_bar_conditions(b)
    report(f"decoder {name}: twin fp16 error masks {b['e16_mask']:.3e} iou {b['e16_iou']:.3e}, bars {b['bar_mask']:.3e} / {b['bar_iou']:.3e}")
    rc, low, iou, _ = decode_dev(name, gpu_device)
    assert rc == 0, _lib.lib().gsr_last_error()
    low64, iou64 = DC.twin(name)
    held(f"decoder {name} masks", low, low64, b["bar_mask"])
    held(f"decoder {name} iou", iou, iou64, b["bar_iou"])
    # two runs give the same bits
    rc, low2, iou2, _ = decode_dev(name, gpu_device)
    assert rc == 0 and torch.equal(low2, low) and torch.equal(iou2, iou)
    if name == "D3":            # a point's bits do not depend on the points that share its call
        pts = DC.points(name)
        for k in (0, 63, 64, 66):
            rc, lo1, io1, _ = decode_dev(name, gpu_device, pts=pts[k:k + 1])
            assert rc == 0 and torch.equal(lo1[0], low[k]) and torch.equal(io1[0], iou[k]), k


# ---------------------------------------------------------------- the generator and the command
def test_generator_with_the_hip_decoder(gpu_device, tmp_path):
    from PIL import Image
    DC.tiny_scan(str(tmp_path / "scan"))
    image = np.asarray(Image.open(str(tmp_path / "scan" / "images" / "0000.png")).convert("RGB"))
    w = DC.weights("D1")
    ref = S.SamMaskGenerator(w, points_per_side=8, device=gpu_device)
    assert ref.decoder == "torch"
    gen = S.SamMaskGenerator(w, points_per_side=8, device=gpu_device, decoder="hip")
    e = ref.embed(image)
    points = S.point_grid(8, e["input_size"])
    low_t, iou_t = ref.decode(e["emb"], points)
    assert ref._hip is None and ref._modules is not None and gen._modules is None      # each ran its own path only
    low, iou = gen.decode(e["emb"], points)
    assert low.shape == (64, 3, 28, 28) and iou.shape == (64, 3) and low.dtype == torch.float32
    b = DC.model_bars("D1")
    # the torch path is fp32 on this embedding: its own distance to fp64 is far inside the bar
    held("generator decode, masks against the torch path", low, low_t.double().cpu(), b["bar_mask"])
    held("generator decode, iou against the torch path", iou, iou_t.double().cpu(), b["bar_iou"])
    # a small workspace budget chunks the points and changes no bit
    budget = S.DECODER_WORKSPACE_BUDGET
    try:
        S.DECODER_WORKSPACE_BUDGET = _lib.lib().gsr_sam_decode_workspace_bytes(7, 5)
        low5, iou5 = gen.decode(e["emb"], points)
    finally:
        S.DECODER_WORKSPACE_BUDGET = budget
    assert torch.equal(low5, low) and torch.equal(iou5, iou)
    gen.pred_iou_thresh, gen.stability_score_thresh, gen.box_nms_thresh = float(iou.median()), 0.0, 1.0
    masks = gen.generate(image)
    assert len(masks) > 0 and set(gen.last_ms) == {"embed", "decode", "select"}
    piou = [m["predicted_iou"] for m in masks]
    assert piou == sorted(piou, reverse=True)
    for m in masks:
        seg = m["segmentation"]
        assert seg.shape == (96, 128) and seg.dtype == bool and m["area"] == int(seg.sum()) > 0
        ys, xs = np.nonzero(seg)
        x, y, bw, bh = m["bbox"]
        assert (x, y, x + bw, y + bh) == (xs.min(), ys.min(), xs.max(), ys.max())
        assert m["crop_box"] == [0, 0, 128, 96] and len(m["point_coords"]) == 1
    with pytest.raises(_lib.GsrError):
        gen.decode(e["emb"].cpu(), points)


def test_sam_cli_with_the_hip_decoder(gpu_device, tmp_path, capsys):
    from gaussmart_amd import sam_cli, segment_cli
    scan, out, ckpt = str(tmp_path / "scan"), str(tmp_path / "out"), str(tmp_path / "ckpt")
    DC.tiny_scan(scan)
    S.save_sam_weights(DC.weights("D1"), ckpt)
    sam_cli.main(["-s", scan, "-o", out, "--views", "1", "0", "--sam_checkpoint", ckpt, "--points_per_side", "4", "--device", str(gpu_device),
                  "--pred_iou_thresh", "-100", "--stability_score_thresh", "0.0", "--decoder", "hip"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["view"] for l in lines] == [1, 0] and all(l["decoder"] == "hip" and l["masks"] > 0 for l in lines)
    for k in range(2):
        with np.load(os.path.join(out, "segments", "masks", f"segments_{k:03d}.npz")) as z:
            assert set(z.files) == {"masks", "boxes", "areas"} and z["masks"].shape[1:] == (96, 128) and len(z["masks"]) == lines[k]["masks"]
    segment_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--masks", os.path.join(out, "segments", "masks"), "--views", "1", "0"])
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert info["points"] == 200 and os.path.exists(os.path.join(out, "segments", "point_cloud", "segment_indices.npy"))


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(gpu_device):
    L = _lib.lib()
    rc, low, iou, h = decode_dev("D1", gpu_device)
    assert rc == 0 and not bool((low == -3.0).any())
    assert L.gsr_sam_dec_num_weights() == h["n"] == _lib.GSR_SAMD_W_COUNT
    tensors = h["tensors"]
    null = (C.c_void_p * len(tensors))(*[None if i == 40 else t.data_ptr() for i, t in enumerate(tensors)])
    for kw in (dict(g=0), dict(g=65), dict(n=h["n"] - 1), dict(table=null), dict(short=256), dict(pts=torch.zeros(0, 2))):
        rc, low, iou, _ = decode_dev("D1", gpu_device, **kw)
        assert rc == -1 and bool((low == -3.0).all()) and bool((iou == -3.0).all()), kw
    assert L.gsr_sam_decode_workspace_bytes(0, 4) == 0 and L.gsr_sam_decode_workspace_bytes(65, 4) == 0
    assert L.gsr_sam_decode_workspace_bytes(7, 0) == 0
    # the stage entry points: no points, a short workspace, a grid that is not built
    o = torch.full((1, 49, 256), -3.0, dtype=torch.float16, device=gpu_device)
    z = torch.zeros(1 << 16, dtype=torch.float16, device=gpu_device)
    ws = workspace(L.gsr_sam_dec_i2t_workspace_bytes(1, 49), gpu_device)
    s = stream(gpu_device)
    assert L.gsr_sam_dec_prompt(ptr(z), 0, 112, ptr(z), ptr(z), ptr(z), ptr(o), s) == -1
    assert L.gsr_sam_dec_t2i(ptr(z), ptr(z), None, ptr(z), 0, 49, 0, ptr(o), s) == -1
    assert L.gsr_sam_dec_t2i(ptr(z), ptr(z), None, ptr(z), 1, 64 * 64 + 1, 0, ptr(o), s) == -1
    assert L.gsr_sam_dec_i2t(*[ptr(z)] * 5, 1, 49, 0, *[ptr(z)] * 4, ptr(ws), 16, ptr(o), s) == -1
    assert L.gsr_sam_dec_upscale(ptr(z), 65, 1, *[ptr(z)] * 7, ptr(ws), ws.numel(), ptr(o), s) == -1
    assert L.gsr_sam_dec_upscale(ptr(z), 7, 1, *[ptr(z)] * 7, ptr(ws), 16, ptr(o), s) == -1
    torch.cuda.synchronize(gpu_device)
    assert bool((o == -3.0).all())
