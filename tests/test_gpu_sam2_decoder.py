"""SAM2's prompt encoder and mask decoder on the kernels (csrc/sam_decoder.hip; include/gsr.h: the SD_* rules with the S2D_*
deltas), everything through the C ABI: the three image-side stages with eight tokens against fp64 restatements of their rules
with bars built from the stated roundings (and named wrong readings that must exceed them tenfold), the eps of layer_norm4,
the whole decoder against transformers' fp64 modules with a bar measured on transformers' own fp16 modules, the bit-equalities,
the generator and sam_cli --sam2 with decoder="hip", and the refusals.  Cases, twins and bars are in
tests/sam2_decoder_cases.py.  GSR_SAM2_DECODER_PARITY_REPORT=<file>: the measured errors and bars are appended there
(profiles/sam2_decoder_parity.txt is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sam2_decoder_cases as KC
from gaussmart_amd import _lib
from gaussmart_amd import sam as S1
from gaussmart_amd import sam2 as S2
from gaussmart_amd._dev import ptr, stream, workspace

pytestmark = pytest.mark.gpu


def report(line):
    out = os.environ.get("GSR_SAM2_DECODER_PARITY_REPORT")
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


# ---------------------------------------------------------------- SD_T2I with eight tokens
def t2i_dev(q, kx, kpe, v, P, T, shared, dev):
    out = torch.full((P, 8, 128), -3.0, dtype=torch.float16, device=dev)
    d = [None if t is None else t.to(dev).contiguous() for t in (q, kx, kpe, v)]
    _lib.check(_lib.lib().gsr_sam2_dec_t2i(ptr(d[0]), ptr(d[1]), None if kpe is None else ptr(d[2]), ptr(d[3]), P, T, int(shared), ptr(out),
                                           stream(dev)))
    return out


@pytest.mark.parametrize("g,P", [(7, 1), (9, 5), (17, 67)])
def test_t2i_against_fp64(gpu_device, g, P):
    T = g * g
    gen = torch.Generator().manual_seed(100 * g + P)
    q = 2.0 * torch.randn(P, 8, 128, generator=gen)
    kpe = torch.randn(T, 128, generator=gen)
    for shared in (False, True):
        shape = (T, 128) if shared else (P, T, 128)
        kx, v = KC.h16(shape, gen), KC.h16(shape, gen)
        got = t2i_dev(q, kx, kpe, v, P, T, shared, gpu_device)
        want, bar = KC.t2i64(q, kx, kpe, v, shared)
        held(f"t2i g{g} P{P} shared{int(shared)}", got, want, bar)
        if not shared:
            moved(f"t2i g{g} P{P}: keys without the positional term", KC.t2i64(q, kx, None, v, shared)[0], want, bar)
            # a point's bits do not depend on the others
            k = P - 1
            alone = t2i_dev(q[k:k + 1], kx[k:k + 1], kpe, v[k:k + 1], 1, T, False, gpu_device)
            assert torch.equal(alone[0], got[k])


# ---------------------------------------------------------------- SD_I2T with eight tokens and its eps
def i2t_dev(d, P, T, shared, eps, dev, out=None):
    """d: qx, qpe, k, v, x, ow, ob, lw, lb on the device; out=None: a fresh sentinel-filled buffer"""
    L = _lib.lib()
    nbytes = L.gsr_sam2_dec_i2t_workspace_bytes(P, T)
    assert nbytes > 0
    ws = workspace(nbytes, dev)
    out = torch.full((P, T, 256), -3.0, dtype=torch.float16, device=dev) if out is None else out
    _lib.check(L.gsr_sam2_dec_i2t(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), P, T, int(shared), ptr(d[5]), ptr(d[6]), ptr(d[7]),
                                  ptr(d[8]), eps, ptr(ws), nbytes, ptr(out), stream(dev)))
    return out


@pytest.mark.parametrize("g,P", [(7, 1), (9, 5), (17, 67)])
def test_i2t_against_fp64(gpu_device, g, P):
    T = g * g
    gen = torch.Generator().manual_seed(200 * g + P)
    qpe, k, v = torch.randn(T, 128, generator=gen), 2.0 * torch.randn(P, 8, 128, generator=gen), torch.randn(P, 8, 128, generator=gen)
    ow, ob = KC.h16((256, 128), gen, 128 ** -0.5), KC.h16((256,), gen, 0.1)
    lw, lb = (0.5 + torch.rand(256, generator=gen)).to(torch.float16), KC.h16((256,), gen, 0.1)
    for shared in (False, True):
        qx = KC.h16((T, 128) if shared else (P, T, 128), gen)
        x = KC.h16((T, 256) if shared else (P, T, 256), gen)
        d = [t.to(gpu_device).contiguous() for t in (qx, qpe, k, v, x, ow, ob, lw, lb)]
        out = i2t_dev(d, P, T, shared, 1e-5, gpu_device)
        want, bar = KC.i2t64(qx, qpe, k, v, x, shared, ow, ob, lw, lb)
        held(f"i2t g{g} P{P} shared{int(shared)}", out, want, bar)
        if not shared:
            moved(f"i2t g{g} P{P}: layer_norm4 left out", KC.i2t64(qx, qpe, k, v, x, shared, ow, ob, lw, lb, norm=False)[0], want, bar)
            # the eighth token is a key: without it the result moves
            moved(f"i2t g{g} P{P}: seven keys", KC.i2t64(qx, qpe, k[:, :7], v[:, :7], x, shared, ow, ob, lw, lb)[0], want, bar)
            # alone, and in place: the same bits
            j = P - 1
            one = [d[0][j:j + 1], d[1], d[2][j:j + 1], d[3][j:j + 1], d[4][j:j + 1]] + d[5:]
            assert torch.equal(i2t_dev(one, 1, T, False, 1e-5, gpu_device)[0], out[j])
            i2t_dev(d, P, T, False, 1e-5, gpu_device, out=d[4])
            assert torch.equal(d[4], out)


def test_i2t_eps_is_1e5(gpu_device):
    """x scaled by 2^-8 and a zero out_proj: the row variance is of the order of eps, so eps decides the result."""
    g, P = 7, 2
    T = g * g
    gen = torch.Generator().manual_seed(77)
    qpe, k, v = torch.randn(T, 128, generator=gen), 2.0 * torch.randn(P, 8, 128, generator=gen), torch.randn(P, 8, 128, generator=gen)
    ow, ob = torch.zeros(256, 128, dtype=torch.float16), torch.zeros(256, dtype=torch.float16)
    lw, lb = (0.5 + torch.rand(256, generator=gen)).to(torch.float16), KC.h16((256,), gen, 0.1)
    qx, x = KC.h16((P, T, 128), gen), KC.h16((P, T, 256), gen, 2.0 ** -8)
    var = float(x.double().var(-1, unbiased=False).mean())
    assert 1e-6 < var < 1e-4, var
    d = [t.to(gpu_device).contiguous() for t in (qx, qpe, k, v, x, ow, ob, lw, lb)]
    out = i2t_dev(d, P, T, False, 1e-5, gpu_device)
    want, bar = KC.i2t64(qx, qpe, k, v, x, False, ow, ob, lw, lb, eps=1e-5)
    held("i2t eps: variance of the order of eps, held at 1e-5", out, want, bar)
    moved("i2t eps: SAM's 1e-6", KC.i2t64(qx, qpe, k, v, x, False, ow, ob, lw, lb, eps=1e-6)[0], want, bar)
    # the argument is what decides: at 1e-6 the kernel follows the other restatement
    out6 = i2t_dev(d, P, T, False, 1e-6, gpu_device)
    held("i2t eps: the argument 1e-6", out6, *KC.i2t64(qx, qpe, k, v, x, False, ow, ob, lw, lb, eps=1e-6))


# ---------------------------------------------------------------- SD_UP with the two skips
@pytest.mark.parametrize("g", [7, 9])
def test_upscale_against_fp64(gpu_device, g):
    P, T, L = 5, g * g, _lib.lib()
    w = KC.weights("K1")
    table = w.decoder_table()
    up = _lib.GSR_SAMD_W_UP
    gen = torch.Generator().manual_seed(300 + g)
    x = KC.h16((P, T, 256), gen)
    s0, s1 = KC.h16((32, 4 * g, 4 * g), gen).float(), KC.h16((64, 2 * g, 2 * g), gen).float()
    hyper4 = torch.randn(P, 4, 32, generator=gen)                      # the four mask tokens' rows; the kernels get 1..3
    hyper = hyper4[:, 1:].permute(1, 0, 2).contiguous()                # [3,P,32]
    nbytes = L.gsr_sam2_dec_upscale_workspace_bytes(g, P)
    assert nbytes > L.gsr_sam_dec_upscale_workspace_bytes(g, P) > 0
    ws = workspace(nbytes, gpu_device)
    out = torch.full((P, 3, 4 * g, 4 * g), -3.0, device=gpu_device)
    d = [t.to(gpu_device).contiguous() for t in [x] + table[up:up + 6] + [hyper, s0, s1]]
    _lib.check(L.gsr_sam2_dec_upscale(ptr(d[0]), g, P, *[ptr(t) for t in d[1:7]], ptr(d[7]), ptr(d[8]), ptr(d[9]), ptr(ws), nbytes, ptr(out),
                                      stream(gpu_device)))
    mod = [w.tensors["mask_decoder." + k].to(torch.float16) for k in S1.DEC_UP]
    want, bar = KC.up64(x, g, *mod, hyper4[:, 1:], s0, s1)
    held(f"upscale g{g}", out, want, bar)
    moved(f"upscale g{g}: feat_s1 added after the LayerNorm", KC.up64(x, g, *mod, hyper4[:, 1:], s0, s1, s1_after_norm=True)[0], want, bar)
    moved(f"upscale g{g}: feat_s0 added after the GELU", KC.up64(x, g, *mod, hyper4[:, 1:], s0, s1, s0_after_gelu=True)[0], want, bar)
    moved(f"upscale g{g}: feat_s0's taps transposed", KC.up64(x, g, *mod, hyper4[:, 1:], s0, s1, swap0=True)[0], want, bar)
    moved(f"upscale g{g}: feat_s1's taps transposed", KC.up64(x, g, *mod, hyper4[:, 1:], s0, s1, swap1=True)[0], want, bar)
    moved(f"upscale g{g}: mask tokens 0..2", KC.up64(x, g, *mod, hyper4[:, :3], s0, s1)[0], want, bar)


# ---------------------------------------------------------------- the whole decoder
def decode_dev(name, dev, pts=None, table=None, n=None, g=None, short=0, P=None, image_size=None, null=()):
    """(rc, low_res, iou, the generator's table) of gsr_sam2_decode on case `name`; null: names of pointers passed as NULL."""
    L = _lib.lib()
    w = KC.weights(name)
    gg = w.config.image_size // 16
    g = gg if g is None else g
    h = S2.Sam2MaskGenerator(w, device=dev, decoder="hip")._decoder_hip()
    pts = KC.points(name) if pts is None else pts
    P = len(pts) if P is None else P
    rows = max(len(pts), 1)
    s0, s1, top = (m.to(dev).contiguous() for m in KC.maps(name))
    p = pts.to(dev).contiguous()
    nbytes = max(L.gsr_sam2_decode_workspace_bytes(gg, rows), 256)
    ws = workspace(nbytes, dev)
    low = torch.full((rows, 3, 4 * gg, 4 * gg), -3.0, device=dev)
    iou = torch.full((rows, 3), -3.0, device=dev)
    a = dict(s0=ptr(s0), s1=ptr(s1), emb=ptr(top), pe=ptr(h["wide"]), points=ptr(p), ws=ptr(ws), low=ptr(low), iou=ptr(iou))
    for k in null:
        a[k] = None
    rc = L.gsr_sam2_decode(g, h["table"] if table is None else table, h["n"] if n is None else n, a["s0"], a["s1"], a["emb"], a["pe"],
                           a["points"], P, 16 * g if image_size is None else image_size, a["ws"], nbytes - short, a["low"], a["iou"],
                           stream(dev))
    torch.cuda.synchronize(dev)
    return rc, low, iou, h


@pytest.mark.parametrize("name", ["K1", "K2"])
def test_decoder_against_the_twin(gpu_device, name):
    b = KC.model_bars(name)
    KC.check_bar_conditions(b)
    report(KC.bars_line(name, b))
    rc, low, iou, _ = decode_dev(name, gpu_device)
    assert rc == 0, _lib.lib().gsr_last_error()
    low64, iou64 = KC.twin(name)
    held(f"decoder {name} masks", low, low64, b["bar_mask"])
    held(f"decoder {name} iou", iou, iou64, b["bar_iou"])
    # two runs give the same bits
    rc, low2, iou2, _ = decode_dev(name, gpu_device)
    assert rc == 0 and torch.equal(low2, low) and torch.equal(iou2, iou)
    if name == "K2":            # a point's bits do not depend on the points that share its call
        pts = KC.points(name)
        for k in (0, 63, 64, 66):
            rc, lo1, io1, _ = decode_dev(name, gpu_device, pts=pts[k:k + 1])
            assert rc == 0 and torch.equal(lo1[0], low[k]) and torch.equal(io1[0], iou[k]), k


# ---------------------------------------------------------------- the generator and the command
def test_generator_with_the_hip_decoder(gpu_device, tmp_path):
    from PIL import Image
    KC.tiny_scan(str(tmp_path / "scan"))
    image = np.asarray(Image.open(str(tmp_path / "scan" / "images" / "0000.png")).convert("RGB"))
    w = KC.weights("K2")
    ref = S2.Sam2MaskGenerator(w, points_per_side=8, device=gpu_device)
    assert ref.decoder == "torch"
    gen = S2.Sam2MaskGenerator(w, points_per_side=8, device=gpu_device, decoder="hip")
    e = ref.embed(image)
    points = S1.point_grid(8, e["input_size"])
    low_t, iou_t = ref.decode(e["emb"], points)
    assert ref._hip is None and ref._modules is not None and gen._modules is None      # each ran its own path only
    low, iou = gen.decode(e["emb"], points)
    assert gen._modules is None and gen._hip is not None
    assert low.shape == (64, 3, 64, 64) and iou.shape == (64, 3) and low.dtype == torch.float32
    b = KC.model_bars("K2")
    # the torch path is fp32 on this embedding: its own distance to fp64 is far inside the bar
    held("generator decode, masks against the torch path", low, low_t.double().cpu(), b["bar_mask"])
    held("generator decode, iou against the torch path", iou, iou_t.double().cpu(), b["bar_iou"])
    # a small workspace budget chunks the points and changes no bit
    budget = S1.DECODER_WORKSPACE_BUDGET
    try:
        S1.DECODER_WORKSPACE_BUDGET = _lib.lib().gsr_sam2_decode_workspace_bytes(16, 5)
        low5, iou5 = gen.decode(e["emb"], points)
    finally:
        S1.DECODER_WORKSPACE_BUDGET = budget
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
        gen.decode([m.cpu() for m in e["emb"]], points)


def test_sam_cli_sam2_with_the_hip_decoder(gpu_device, tmp_path, capsys):
    from gaussmart_amd import sam_cli, segment_cli
    scan, out, ckpt = str(tmp_path / "scan"), str(tmp_path / "out"), str(tmp_path / "ckpt")
    KC.tiny_scan(scan)
    S2.save_sam2_weights(KC.weights("K1"), ckpt)
    sam_cli.main(["--sam2", "-s", scan, "-o", out, "--views", "1", "0", "--sam_checkpoint", ckpt, "--points_per_side", "4", "--device",
                  str(gpu_device), "--pred_iou_thresh", "-100", "--stability_score_thresh", "0.0", "--decoder", "hip"])
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
    rc, low, iou, h = decode_dev("K1", gpu_device)
    assert rc == 0 and not bool((low == -3.0).any()) and not bool((iou == -3.0).any())
    assert L.gsr_sam2_dec_num_weights() == h["n"] == _lib.GSR_SAM2D_W_COUNT == 119
    tensors = h["tensors"]
    null_entry = (C.c_void_p * len(tensors))(*[None if i == 40 else t.data_ptr() for i, t in enumerate(tensors)])
    null_last = (C.c_void_p * len(tensors))(*[None if i == 118 else t.data_ptr() for i, t in enumerate(tensors)])
    cases = [dict(g=0), dict(g=65), dict(pts=torch.zeros(0, 2)), dict(P=65536), dict(image_size=16 * 8 + 1), dict(image_size=64),
             dict(n=h["n"] - 1), dict(n=h["n"] + 1), dict(table=null_entry), dict(table=null_last), dict(short=256)]
    cases += [dict(null=(k,)) for k in ("s0", "s1", "emb", "pe", "points", "ws", "low", "iou")]
    for kw in cases:
        rc, low, iou, _ = decode_dev("K1", gpu_device, **kw)
        assert rc == -1 and bool((low == -3.0).all()) and bool((iou == -3.0).all()), kw
    for f in (L.gsr_sam2_decode_workspace_bytes, L.gsr_sam2_dec_upscale_workspace_bytes):
        assert f(0, 4) == 0 and f(65, 4) == 0 and f(7, 0) == 0 and f(7, 65536) == 0 and f(7, 4) > 0
    f = L.gsr_sam2_dec_i2t_workspace_bytes
    assert f(0, 49) == 0 and f(65536, 49) == 0 and f(1, 0) == 0 and f(1, 64 * 64 + 1) == 0 and f(1, 49) > 0
    # the stage entry points: no points, a short workspace, a grid that is not built, a null pointer
    o = torch.full((1, 49, 256), -3.0, dtype=torch.float16, device=gpu_device)
    z = torch.zeros(1 << 17, dtype=torch.float16, device=gpu_device)
    ws = workspace(max(L.gsr_sam2_dec_i2t_workspace_bytes(1, 49), L.gsr_sam2_dec_upscale_workspace_bytes(7, 1)), gpu_device)
    s, n = stream(gpu_device), ws.numel() * ws.element_size()
    assert L.gsr_sam2_dec_t2i(ptr(z), ptr(z), None, ptr(z), 0, 49, 0, ptr(o), s) == -1
    assert L.gsr_sam2_dec_t2i(ptr(z), ptr(z), None, ptr(z), 1, 64 * 64 + 1, 0, ptr(o), s) == -1
    assert L.gsr_sam2_dec_t2i(ptr(z), None, None, ptr(z), 1, 49, 0, ptr(o), s) == -1
    assert L.gsr_sam2_dec_i2t(*[ptr(z)] * 5, 1, 49, 0, *[ptr(z)] * 4, 1e-5, ptr(ws), 16, ptr(o), s) == -1
    assert L.gsr_sam2_dec_i2t(*[ptr(z)] * 5, 0, 49, 0, *[ptr(z)] * 4, 1e-5, ptr(ws), n, ptr(o), s) == -1
    assert L.gsr_sam2_dec_i2t(*[ptr(z)] * 5, 1, 49, 0, *[ptr(z)] * 4, 0.0, ptr(ws), n, ptr(o), s) == -1
    assert L.gsr_sam2_dec_i2t(*[ptr(z)] * 4, None, 1, 49, 0, *[ptr(z)] * 4, 1e-5, ptr(ws), n, ptr(o), s) == -1
    assert L.gsr_sam2_dec_upscale(ptr(z), 65, 1, *[ptr(z)] * 9, ptr(ws), n, ptr(o), s) == -1
    assert L.gsr_sam2_dec_upscale(ptr(z), 7, 1, *[ptr(z)] * 9, ptr(ws), 16, ptr(o), s) == -1
    assert L.gsr_sam2_dec_upscale(ptr(z), 7, 1, *[ptr(z)] * 7, None, ptr(z), ptr(ws), n, ptr(o), s) == -1
    assert L.gsr_sam2_dec_upscale(ptr(z), 7, 1, *[ptr(z)] * 8, None, ptr(ws), n, ptr(o), s) == -1
    torch.cuda.synchronize(gpu_device)
    assert bool((o == -3.0).all())
