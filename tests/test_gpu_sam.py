"""The SAM kernels (csrc/sam.hip; include/gsr.h: SV_EMBED, SV_ATTN, SV_NECK, SM_SCORE, SM_NMS, SM_EMIT) on the device,
everything through the C ABI: each encoder stage against fp64 from the same fp16 inputs with a bar that follows the roundings
its rule states, the whole encoder against transformers' fp64 model with a bar measured on transformers' own fp16 model, the
mask selection against the fp64 torch formulation pixel by pixel wherever that formulation decides, the NMS against a plain
loop, the generator end to end, the bit-equalities, the refusals, and sam_cli feeding segment_cli.  Cases, twins and the bar
arithmetic are in tests/sam_cases.py.  GSR_SAM_PARITY_REPORT=<file>: the measured errors and bars are appended there
(profiles/sam_parity.txt is such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sam_cases as SC
from sam_cases import U16, U32
from gaussmart_amd import _lib
from gaussmart_amd import sam as S
from gaussmart_amd._dev import ptr, stream, workspace

pytestmark = pytest.mark.gpu


def report(line):
    out = os.environ.get("GSR_SAM_PARITY_REPORT")
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


# ---------------------------------------------------------------- SV_EMBED
@pytest.mark.parametrize("S_,hidden", [(112, 128), (144, 320)])
def test_embed_against_fp64(gpu_device, S_, hidden):
    g = torch.Generator().manual_seed(S_ + hidden)
    gr = S_ // 16
    x = torch.randn(3, S_, S_, generator=g)
    pw, pb, pos = h16((hidden, 768), g, 768 ** -0.5), h16((hidden,), g, 0.1), h16((gr, gr, hidden), g)
    L = _lib.lib()
    nbytes = L.gsr_sam_embed_workspace_bytes(S_)
    ws = workspace(nbytes, gpu_device)
    out = torch.full((gr * gr, hidden), float("nan"), device=gpu_device)
    d = [t.to(gpu_device) for t in (x, pw, pb, pos)]
    _lib.check(L.gsr_sam_embed(ptr(d[0]), S_, hidden, ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(ws), nbytes, ptr(out), stream(gpu_device)))
    x16 = x.to(torch.float16).double()
    patches = x16.reshape(3, gr, 16, gr, 16).permute(1, 3, 0, 2, 4).reshape(gr * gr, 768)
    u = patches @ pw.double().T + pb.double()
    want = u + pos.double().reshape(gr * gr, hidden)
    # the fp32 chain of 768 terms, the bias addition and the position addition (one fp32 rounding each)
    bar = 768 * U32 * (patches.abs() @ pw.double().abs().T) + U32 * u.abs() + U32 * want.abs() + 2 * U32
    held(f"embed S{S_} h{hidden}", out, want, bar)


# ---------------------------------------------------------------- SV_ATTN
def attn_dev(qkv, bias, Rh, Rw, g, w, heads, hd, dev):
    L = _lib.lib()
    nbytes = L.gsr_sam_attn_workspace_bytes(g, w, heads)
    ws = workspace(nbytes, dev)
    out = torch.full((g * g, heads * hd), float("nan"), dtype=torch.float16, device=dev)
    d = [t.to(dev) for t in (qkv, bias, Rh, Rw)]
    _lib.check(L.gsr_sam_attn(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), Rh.shape[0], g, w, heads, hd, ptr(ws), nbytes, ptr(out), stream(dev)))
    return out


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("g,w", [(7, 3), (9, 4), (17, 14), (7, 0), (17, 0)])
def test_attention_against_fp64(gpu_device, g, w, hd):
    heads, s = 2, (g if w == 0 else w)
    gen = torch.Generator().manual_seed(100 * g + w + hd)
    qkv, bias = h16((g * g, 3 * heads * hd), gen), h16((3 * heads * hd,), gen)
    Rh, Rw = h16((2 * s - 1, hd), gen, hd ** -0.5), h16((2 * s - 1, hd), gen, hd ** -0.5)
    want, bar = SC.attention64(qkv, bias, Rh, Rw, g, w, heads, hd)
    got = attn_dev(qkv, bias, Rh, Rw, g, w, heads, hd, gpu_device)
    held(f"attn g{g} w{w} hd{hd}", got, want, bar)
    # the same bits again, and the q third of the bias (which no padded key uses) changes nothing
    bias2 = bias.clone()
    bias2[:heads * hd] = 7.0
    assert torch.equal(attn_dev(qkv, bias2, Rh, Rw, g, w, heads, hd, gpu_device), got)
    if w:
        # the padded keys are real: without the k and v thirds of the bias the output moves far beyond the bar
        zero = attn_dev(qkv, torch.zeros_like(bias), Rh, Rw, g, w, heads, hd, gpu_device)
        assert float((zero.double().cpu() - want).abs().max()) > 10 * float(bar.max())


# ---------------------------------------------------------------- SV_NECK
@pytest.mark.parametrize("g,hidden", [(7, 128), (9, 320)])
def test_neck_against_fp64(gpu_device, g, hidden):
    Cn, T, eps = 64, g * g, 1e-6
    gen = torch.Generator().manual_seed(g + hidden)
    x = 2.0 * torch.randn(T, hidden, generator=gen)
    w1, w2 = h16((Cn, hidden), gen, hidden ** -0.5), h16((Cn, Cn, 3, 3), gen, (9 * Cn) ** -0.5)
    g1, b1, g2, b2 = ((0.5 + torch.rand(Cn, generator=gen)).to(torch.float16) if i % 2 == 0 else h16((Cn,), gen, 0.1) for i in range(4))
    L = _lib.lib()
    nbytes = L.gsr_sam_neck_workspace_bytes(g, hidden, Cn)
    ws = workspace(nbytes, gpu_device)
    out = torch.full((Cn, g, g), float("nan"), device=gpu_device)
    d = [t.to(gpu_device) for t in (x, w1, g1, b1, w2, g2, b2)]
    _lib.check(L.gsr_sam_neck(ptr(d[0]), g, hidden, Cn, *[ptr(t) for t in d[1:]], ptr(ws), nbytes, ptr(out), stream(gpu_device)))

    def norm(c, gam, beta):
        mean = c.mean(1, keepdim=True)
        dlt = c - mean
        rstd = 1.0 / torch.sqrt((dlt * dlt).mean(1, keepdim=True) + eps)
        z = dlt * rstd
        return z * gam.double() + beta.double(), z, rstd

    def norm_err(dc, z, rstd, gam, y, n):
        # first order: dz_i = rstd (dc_i - mean dc - z_i mean(z dc)), so |dz_i| <= rstd max|dc| (2 + |z_i|) as mean|z| <= 1;
        # DN_NORM's own fp32 roundings: (n + 16) 2^-24 on the statistics and the four operations of the output
        own = (n + 16) * U32 * (z.abs() * gam.double().abs() + y.abs())
        return gam.double().abs() * rstd * dc.max(1, keepdim=True).values * (2 + z.abs()) + own

    # the same fp16 inputs: the stream rounded to fp16 is part of the rule
    x16 = x.to(torch.float16).double()
    c1 = x16 @ w1.double().T
    e1 = hidden * U32 * (x16.abs() @ w1.double().abs().T)
    y1, z1, r1 = norm(c1, g1, b1)
    ey1 = norm_err(e1, z1, r1, g1, y1, Cn)
    ey1 = ey1 + SC.round16(y1, ey1)
    y1h = torch.nn.functional.pad(y1.reshape(g, g, Cn), (0, 0, 1, 1, 1, 1))
    e1h = torch.nn.functional.pad(ey1.reshape(g, g, Cn), (0, 0, 1, 1, 1, 1))
    col = torch.stack([y1h[ky:ky + g, kx:kx + g] for ky in range(3) for kx in range(3)], -1).reshape(T, Cn * 9)
    ecol = torch.stack([e1h[ky:ky + g, kx:kx + g] for ky in range(3) for kx in range(3)], -1).reshape(T, Cn * 9)
    w2m = w2.double().reshape(Cn, Cn * 9)
    c2 = col @ w2m.T
    # conv2 is linear in its input: the input's error through |w|, plus the fp32 chain of 9 C terms
    e2 = ecol @ w2m.abs().T + 9 * Cn * U32 * ((col.abs() + ecol) @ w2m.abs().T)
    y2, z2, r2 = norm(c2, g2, b2)
    bar = norm_err(e2, z2, r2, g2, y2, Cn)
    held(f"neck g{g} h{hidden}", out.reshape(Cn, T).T, y2, bar)
    # the bar is a worst-case bound; it must still tell a wrong k order of the 3x3 product apart
    wrong = (col.reshape(T, Cn, 9).transpose(1, 2).reshape(T, 9 * Cn) @ w2m.T)
    assert float((norm(wrong, g2, b2)[0] - y2).abs().max()) > 10 * float(bar.max())


# ---------------------------------------------------------------- the whole encoder
@pytest.fixture(scope="module")
def encoders():
    return {}


def encode(name, dev, encoders):
    if name not in encoders:
        encoders[name] = S.SamImageEncoder(SC.weights(name))
    return encoders[name].encode(SC.pixels(name).to(dev))


@pytest.mark.parametrize("name", ["E1", "E2", "E3"])
def test_encoder_against_the_twin(gpu_device, name, encoders):
    bars = SC.model_bars(name)
    report(f"encoder {name}: twin fp16 error {bars['e16']:.3e}, bar {bars['bar']:.3e}, no rel-pos moves {bars['no_rel']:.3e}, "
           f"masked padded keys move {bars['masked_pad']:.3e}")
    SC.check_bar_conditions(bars)
    got = encode(name, gpu_device, encoders)
    cfg = SC.config(name)
    assert got.shape == (cfg.output_channels, cfg.grid, cfg.grid) and got.dtype == torch.float32
    held(f"encoder {name}", got, SC.twin(name), bars["bar"])
    assert torch.equal(encode(name, gpu_device, encoders), got)           # the same bits on every run


# ---------------------------------------------------------------- SM_SCORE / SM_EMIT
def score_dev(logits, input_size, mask_size, dev, skip=None, tau=0.0, delta=1.0):
    n, Lr = logits.shape[0], logits.shape[-1]
    counts = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
    boxes = torch.full((n, 4), -7.0, device=dev)
    _lib.check(_lib.lib().gsr_sam_mask_score(ptr(logits), n, Lr, *input_size, *mask_size, tau, delta, ptr(skip), ptr(counts), ptr(boxes),
                                             stream(dev)))
    return counts, boxes


def emit_dev(logits, input_size, mask_size, index, dev, tau=0.0):
    n, Lr, m = logits.shape[0], logits.shape[-1], len(index)
    out = torch.full((m, *mask_size), 9, dtype=torch.uint8, device=dev)
    idx = torch.as_tensor(index, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().gsr_sam_mask_emit(ptr(logits), n, Lr, *input_size, *mask_size, tau, ptr(idx), m, ptr(out), stream(dev)))
    return out


MASK_SHAPES = [(40, (120, 160), (120, 160), 24), (40, (160, 120), (213, 160), 24), (40, (120, 160), (73, 97), 24),
               (64, (256, 171), (1000, 668), 200)]


@pytest.mark.parametrize("Lr,input_size,mask_size,n", MASK_SHAPES)
def test_mask_score_and_emit_against_fp64(gpu_device, Lr, input_size, mask_size, n):
    logits = SC.mask_logits(Lr, *input_size, n=n)
    truth = SC.mask_truth(logits, input_size, mask_size)
    dl = logits.to(gpu_device)
    counts, boxes = score_dev(dl, input_size, mask_size, gpu_device)
    planes = emit_dev(dl, input_size, mask_size, list(range(n)), gpu_device)
    # the bit-equalities: the same bits twice, and every plane's pixel count is SM_SCORE's area
    again = score_dev(dl, input_size, mask_size, gpu_device)
    assert torch.equal(again[0], counts) and torch.equal(again[1], boxes)
    assert torch.equal(planes.flatten(1).sum(1, dtype=torch.int32), counts[:, 0]) and int(planes.max()) <= 1
    planes, counts, boxes = planes.cpu().bool(), counts.cpu().long(), boxes.cpu()
    on, decided = truth["on"], truth["decided"]
    und = (~decided).flatten(1).sum(1)
    share = float(und.sum()) / decided.numel()
    flips = int(((planes != on) & decided).sum())
    worst = int(((counts - truth["counts"]).abs().max(1).values - und).max())
    report(f"masks L{Lr} {input_size}->{mask_size} n{n}: undecided share {share:.2e}, decided pixels that differ {flips}, "
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
    report(f"masks L{Lr} {input_size}->{mask_size} n{n}: {checked} boxes had no undecided pixel outside them and were compared exactly")
    assert checked >= 2                                            # the constant masks at the least
    # the empty and the full mask; the empty one is rejected (0 / 0)
    assert counts[0].tolist() == [0, 0, 0] and boxes[0].tolist() == [0, 0, 0, 0]
    assert counts[1].tolist() == [H * W] * 3 and boxes[1].tolist() == [0, 0, W - 1, H - 1]
    stab = counts[:, 1].float() / counts[:, 2].float()
    assert not bool(stab[0] >= 0.92) and bool(stab[1] >= 0.92)
    # a skipped mask is not read (its logits are NaN here) and reports zeros; the others keep their bits
    skip = torch.zeros(n, dtype=torch.uint8, device=gpu_device)
    skip[3] = 1
    poisoned = dl.clone()
    poisoned[3] = float("nan")
    c2, b2 = score_dev(poisoned, input_size, mask_size, gpu_device, skip)
    keep = torch.arange(n) != 3
    assert c2[3].tolist() == [0, 0, 0] and b2[3].tolist() == [0, 0, 0, 0]
    assert torch.equal(c2.cpu().long()[keep], counts[keep]) and torch.equal(b2.cpu()[keep], boxes[keep])
    # SM_EMIT of a list: the planes of those masks in that order; an index outside the masks is a zero plane
    some = emit_dev(dl, input_size, mask_size, [5, 1, n, 2], gpu_device).cpu().bool()
    assert torch.equal(some[0], planes[5]) and torch.equal(some[1], planes[1]) and not some[2].any() and torch.equal(some[3], planes[2])


def test_stability_verdicts_against_fp64(gpu_device):
    Lr, input_size, mask_size, n, thr = 40, (120, 160), (120, 160), 24, 0.92
    logits = SC.mask_logits(Lr, *input_size, n=n, amp=(20.0, 60.0), seed=1)
    truth = SC.mask_truth(logits, input_size, mask_size)
    inter, union = truth["counts"][:, 1].double(), truth["counts"][:, 2].double()
    s64 = inter / union
    above, below = int((s64 >= thr).sum()), int((~(s64 >= thr)).sum())
    report(f"stability inputs: {above} of {n} masks at or above {thr} in fp64, {below} below")
    assert above >= n // 4 and below >= n // 4                      # about the inputs: both verdicts are exercised
    counts, _ = score_dev(logits.to(gpu_device), input_size, mask_size, gpu_device)
    got = (counts[:, 1].float() / counts[:, 2].float()).cpu() >= thr
    und = (~truth["decided"]).flatten(1).sum(1).double()
    lo, hi = (inter - und).clamp(min=0) / (union + und), (inter + und) / (union - und).clamp(min=1)
    firm = (lo >= thr) | (hi < thr) | (union == 0)
    assert torch.equal(got[firm], (s64 >= thr)[firm]) and int(firm.sum()) >= n - 4


# ---------------------------------------------------------------- SM_NMS
def nms_dev(boxes, scores, keep, theta, dev):
    n = len(scores)
    L = _lib.lib()
    nbytes = L.gsr_sam_nms_workspace_bytes(n)
    ws = workspace(nbytes, dev)
    kept = torch.full((n,), -1, dtype=torch.int32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    k8 = None if keep is None else keep.to(torch.uint8).to(dev)
    db, ds = boxes.to(dev), scores.to(dev)              # held until the call has run
    _lib.check(L.gsr_sam_nms(ptr(db), ptr(ds), ptr(k8), n, theta, ptr(ws), nbytes, ptr(kept), ptr(count), stream(dev)))
    m = int(count.item())
    assert (kept[m:] == -1).all()
    return kept[:m].tolist()


@pytest.mark.parametrize("n,clustered", [(300, False), (1, False), (3 * 64 * 64, True)])
def test_nms_against_the_loop(gpu_device, n, clustered):
    boxes, scores = SC.random_boxes(n, 77 + n, extent=200.0 if n < 1000 else 1500.0, clustered=clustered)
    keep = None
    if n > 10:
        boxes[5] = boxes[6] = torch.tensor([3.0, 3.0, 3.0, 9.0])            # zero area: NaN IoU with each other, both kept
        scores[5] = scores[6] = 2.0
        keep = torch.rand(n, generator=torch.Generator().manual_seed(n)) > 0.1
        keep[5] = keep[6] = True
    for theta in (0.7, 0.3):
        want = SC.nms_loop(boxes.numpy(), scores.numpy(), None if keep is None else keep.numpy(), theta)
        got = nms_dev(boxes, scores, keep, theta, gpu_device)
        report(f"nms n{n} theta{theta}: kept {len(got)} of {n if keep is None else int(keep.sum())}")
        assert got == want                                          # indices and order are exact
    if n > 10:
        assert got[:2] == [5, 6] and 0 < len(got) < n


# ---------------------------------------------------------------- the generator end to end
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
    return pts, [{k.rsplit("_", 1)[0]: v for k, v in mats.items() if k.endswith(f"_{i}")} for i in range(2)]


def test_generator_end_to_end(gpu_device, tmp_path):
    from PIL import Image
    from gaussmart_amd import segment_init as SI
    pts, cams = tiny_scan(str(tmp_path / "scan"))
    image = np.asarray(Image.open(str(tmp_path / "scan" / "images" / "0000.png")).convert("RGB"))
    w = SC.weights("E1", 256)
    gen = S.SamMaskGenerator(w, points_per_side=8, device=gpu_device)
    e = gen.embed(image)
    assert e["emb"].shape == (1, 256, 7, 7) and e["input_size"] == (84, 112) and e["mask_size"] == (96, 128)
    points = S.point_grid(8, e["input_size"])
    low, iou = gen.decode(e["emb"], points)
    assert low.shape == (64, 3, 28, 28) and iou.shape == (64, 3) and torch.isfinite(low).all()
    # thresholds: the medians of this run's own iou and fp64 stability scores
    truth = SC.mask_truth(low.reshape(-1, 28, 28).cpu(), e["input_size"], e["mask_size"])
    s64 = truth["counts"][:, 1].double() / truth["counts"][:, 2].double()
    gen.pred_iou_thresh = float(iou.median())
    gen.stability_score_thresh = float(s64[~torch.isnan(s64)].median())
    sel = gen.select(low, iou, e["input_size"], e["mask_size"])
    host = S.select_host(low, iou, e["input_size"], e["mask_size"], gen.pred_iou_thresh, gen.stability_score_thresh,
                         gen.stability_score_offset, gen.box_nms_thresh, dtype=torch.float64)
    # the two agree on every candidate that is decided: no undecided pixel, and the stability gate away from its threshold
    und = (~truth["decided"]).flatten(1).sum(1)
    inter, union = truth["counts"][:, 1].double(), truth["counts"][:, 2].double()
    lo, hi = (inter - und).clamp(min=0) / (union + und), (inter + und) / (union - und).clamp(min=1)
    firm = ((lo >= gen.stability_score_thresh) | (hi < gen.stability_score_thresh) | (union == 0)).to(gpu_device)
    report(f"generator: {int(sel['keep_in'].sum())} of {len(firm)} candidates pass both gates, {len(sel['index'])} masks after NMS, "
           f"{int((~firm).sum())} candidates undecided")
    assert torch.equal(sel["keep_in"][firm], host["keep_in"][firm]) and 0 < len(sel["index"]) < 192
    if bool(firm.all()) and int(und.sum()) == 0:
        assert torch.equal(sel["index"], host["index"]) and torch.equal(sel["masks"], host["masks"])
        assert torch.equal(sel["boxes"], host["boxes"]) and torch.equal(sel["area"], host["area"])
    # the reference's list of dicts
    # (random decoder weights give near-identical boxes, so NMS at 0.7 leaves very few; with a threshold no IoU exceeds,
    # every candidate that passed the two gates comes out, which is what the order and the fields are checked on)
    gen2 = S.SamMaskGenerator(w, points_per_side=8, pred_iou_thresh=gen.pred_iou_thresh,
                              stability_score_thresh=gen.stability_score_thresh, box_nms_thresh=1.0, device=gpu_device)
    masks = gen2.generate(image)
    assert len(masks) == int(sel["keep_in"].sum()) > 8 and set(gen2.last_ms) == {"embed", "decode", "select"}
    assert [m["predicted_iou"] for m in masks[:len(sel["index"])]][:1] == [float(sel["predicted_iou"][0])]
    piou = [m["predicted_iou"] for m in masks]
    assert piou == sorted(piou, reverse=True)                      # NMS order: descending predicted_iou
    for k, m in enumerate(masks):
        seg = m["segmentation"]
        assert seg.shape == (96, 128) and seg.dtype == bool and m["area"] == int(seg.sum()) > 0
        ys, xs = np.nonzero(seg)
        x, y, bw, bh = m["bbox"]
        assert (x, y, x + bw, y + bh) == (xs.min(), ys.min(), xs.max(), ys.max())
        assert m["crop_box"] == [0, 0, 128, 96] and m["stability_score"] >= gen.stability_score_thresh
        assert m["predicted_iou"] > gen.pred_iou_thresh and len(m["point_coords"]) == 1
    S.save_segments_boxes(masks, str(tmp_path / "seg" / "segments_000.npz"))
    with np.load(str(tmp_path / "seg" / "segments_000.npz")) as z:
        assert set(z.files) == {"masks", "boxes", "areas"} and z["masks"].shape == (len(masks), 96, 128)
        assert np.array_equal(z["areas"], z["masks"].reshape(len(masks), -1).sum(1))
        assert np.array_equal(z["boxes"][:, 2] - z["boxes"][:, 0], [m["bbox"][2] for m in masks])
    # the device tensor is what label_points takes, in the same order
    dev_masks = gen2.generate_device(image)
    assert dev_masks.is_cuda and dev_masks.dtype == torch.uint8 and np.array_equal(dev_masks.cpu().numpy().astype(bool), np.array([m["segmentation"] for m in masks]))
    labels, areas = SI.label_points(pts, cams[:1], "dtu", [dev_masks], device=gpu_device)
    assert labels.shape == (200,) and int(labels.max()) < len(masks)


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing(gpu_device):
    L = _lib.lib()
    w = SC.weights("E1").to(gpu_device)
    cfg = w.config
    tensors = w.table()
    x = SC.pixels("E1").to(gpu_device)

    def call(hidden=cfg.hidden_size, heads=2, head_dim=64, mlp=cfg.mlp_dim, rows=None, short=0, null=None):
        layers = cfg.num_hidden_layers
        windows = (C.c_int32 * layers)(*cfg.windows())
        rel_rows = (C.c_int32 * layers)(*(rows or [5, 13]))
        c = _lib.GsrSamConfig(hidden, heads, head_dim, layers, mlp, cfg.output_channels, cfg.image_size, cfg.layer_norm_eps, windows, rel_rows)
        table = (C.c_void_p * len(tensors))(*[None if i == null else t.data_ptr() for i, t in enumerate(tensors)])
        good = _lib.GsrSamConfig(cfg.hidden_size, 2, 64, layers, cfg.mlp_dim, cfg.output_channels, cfg.image_size, cfg.layer_norm_eps,
                                 windows, (C.c_int32 * layers)(5, 13))
        nbytes = L.gsr_sam_workspace_bytes(C.byref(good))
        assert nbytes > 0
        ws = workspace(nbytes, gpu_device)
        out = torch.full((cfg.output_channels, cfg.grid, cfg.grid), -3.0, device=gpu_device)
        rc = L.gsr_sam_encode(C.byref(c), table, len(tensors), ptr(x), ptr(ws), nbytes - short, ptr(out), stream(gpu_device))
        torch.cuda.synchronize(gpu_device)
        return rc, bool((out == -3.0).all()), L.gsr_sam_workspace_bytes(C.byref(c))

    assert call()[:2] == (0, False)
    for kw in (dict(head_dim=48, heads=2, hidden=96), dict(hidden=192), dict(rows=[5, 12]), dict(rows=[7, 13]), dict(mlp=cfg.mlp_dim + 32),
               dict(short=256), dict(null=4), dict(null=len(tensors) - 1)):
        rc, untouched, nbytes = call(**kw)
        assert rc == -1 and untouched, kw                           # GSR_E_INVALID, and the output is still at its fill value
        if "short" not in kw and "null" not in kw:
            assert nbytes == 0, kw
    # a weight table of the wrong length
    table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    layers = cfg.num_hidden_layers
    keep = ((C.c_int32 * layers)(*cfg.windows()), (C.c_int32 * layers)(5, 13))
    c = _lib.GsrSamConfig(cfg.hidden_size, 2, 64, layers, cfg.mlp_dim, cfg.output_channels, cfg.image_size, cfg.layer_norm_eps, *keep)
    out = torch.full((4,), -3.0, device=gpu_device)
    assert L.gsr_sam_encode(C.byref(c), table, len(tensors) - 1, ptr(x), ptr(out), 16, ptr(out), stream(gpu_device)) == -1
    # the stage entry points: a table of the wrong length, a head dimension that is not built, a short workspace
    q = torch.zeros(49, 384, dtype=torch.float16, device=gpu_device)
    o = torch.full((49, 128), -3.0, dtype=torch.float16, device=gpu_device)
    ws = workspace(L.gsr_sam_attn_workspace_bytes(7, 3, 2), gpu_device)
    for rows, hd, nb in ((6, 64, ws.numel()), (5, 48, ws.numel()), (5, 64, 8)):
        assert L.gsr_sam_attn(ptr(q), ptr(q), ptr(q), ptr(q), rows, 7, 3, 2, hd, ptr(ws), nb, ptr(o), stream(gpu_device)) == -1
    torch.cuda.synchronize(gpu_device)
    assert bool((o == -3.0).all()) and bool((out == -3.0).all())
    assert L.gsr_sam_nms(ptr(q), ptr(q), None, 3 * 64 * 64 + 1, 0.7, ptr(ws), ws.numel(), ptr(q), ptr(q), stream(gpu_device)) == -1
    assert L.gsr_sam_mask_score(ptr(q), 1, 40, 161, 100, 10, 10, 0.0, 1.0, None, ptr(q), ptr(q), stream(gpu_device)) == -1
    with pytest.raises(_lib.GsrError):
        S.SamImageEncoder(SC.weights("E1")).encode(SC.pixels("E1"))          # a host tensor


# ---------------------------------------------------------------- sam_cli -> segment_cli
def test_sam_cli_feeds_segment_cli(gpu_device, tmp_path, capsys):
    from gaussmart_amd import sam_cli, segment_cli
    scan, out, ckpt = str(tmp_path / "scan"), str(tmp_path / "out"), str(tmp_path / "ckpt")
    tiny_scan(scan)
    S.save_sam_weights(SC.weights("E1", 256), ckpt)
    # random weights predict no iou near 0.86: the gates are opened so that the files hold masks
    sam_cli.main(["-s", scan, "-o", out, "--views", "1", "0", "--sam_checkpoint", ckpt, "--points_per_side", "4", "--device", str(gpu_device),
                  "--pred_iou_thresh", "-100", "--stability_score_thresh", "0.0"])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["view"] for l in lines] == [1, 0] and all({"masks", "embed_ms", "decode_ms", "select_ms"} <= set(l) for l in lines)
    assert sorted(os.listdir(os.path.join(out, "segments", "images"))) == ["0000.png", "0001.png"]
    for k in range(2):
        with np.load(os.path.join(out, "segments", "masks", f"segments_{k:03d}.npz")) as z:
            assert set(z.files) == {"masks", "boxes", "areas"} and z["masks"].shape[1:] == (96, 128) and len(z["masks"]) == lines[k]["masks"]
    assert all(l["masks"] > 0 for l in lines)
    segment_cli.main(["-s", scan, "-o", out, "-t", "dtu", "--masks", os.path.join(out, "segments", "masks"), "--views", "1", "0"])
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert info["points"] == 200 and os.path.exists(os.path.join(out, "segments", "point_cloud", "segment_indices.npy"))
