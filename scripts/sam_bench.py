"""Time SAM mask generation on one GPU: the encoder kernels of csrc/sam.hip stage by stage and as a whole at 1024x1024 next to
transformers' SamVisionEncoder in fp32 (the reference's precision) and in fp16 on the same GPU, the mask selection next to
its torch twin, the decoder kernels of csrc/sam_decoder.hip stage by stage and as a whole for 1024 points next to decode_host
in fp32 and in fp16, and an image's time split into embed / decode / select with either decoder.

    python scripts/sam_bench.py [--out profiles/sam_bench.txt] [--model_type vit_h] [--points_per_side 32]

Random weights (gaussmart_amd.sam.random_sam_weights) and seeded inputs: nothing outside the repository is read.  Every
figure is the median of `--repeats` timed calls (device events around one call each, after `--warmup` untimed calls of the
same shape); the spread (min .. max) is printed beside it.  TFLOP/s are the useful operations counted from the shapes over
that time: a rate the call reached, not a share of peak.  These figures are reported, not gated: entries slower than torch's
stay in the table."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                           # noqa: E402
import torch                                                 # noqa: E402

from gaussmart_amd import _lib, sam as S                     # noqa: E402
from gaussmart_amd._dev import ptr, stream, workspace       # noqa: E402


def timed(fn, dev, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fmt(name, t, flop=None):
    med, lo, hi = t
    rate = f"  {flop / med / 1e9:8.1f} TFLOP/s" if flop else ""
    return f"  {name:<52s} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f}){rate}"


def attempt(out, name, fn, dev, args, flop=None):
    try:
        with torch.no_grad():
            t = timed(fn, dev, args.warmup, args.repeats)
        out(fmt(name, t, flop))
        return t[0]
    except Exception as e:          # one entry that fails must not lose the others
        out(f"  {name:<52s} failed: {type(e).__name__}: {e}")
        return None


def stages(cfg, w, dev, args, out):
    L, s, chk = _lib.lib(), stream(dev), _lib.check
    hid, heads, hd, mlp, Cn, g = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.mlp_dim, cfg.output_channels, cfg.grid
    T = g * g
    gen = torch.Generator().manual_seed(0)
    h16 = lambda *shape: torch.randn(*shape, generator=gen).to(torch.float16).to(dev)
    t = w.to(dev).tensors
    glob = cfg.windows().index(0) if 0 in cfg.windows() else None
    win = next((l for l, v in enumerate(cfg.windows()) if v), None)
    x = torch.randn(3, cfg.image_size, cfg.image_size, generator=gen).to(dev)
    resid = torch.randn(T, hid, generator=gen).to(dev)
    xn, qkv, att, act = h16(T, hid), h16(T, 3 * hid), h16(T, hid), h16(T, mlp)
    emb, feat = torch.empty(T, hid, device=dev), torch.empty(Cn, g, g, device=dev)
    ws_e = workspace(L.gsr_sam_embed_workspace_bytes(cfg.image_size), dev)
    ws_n = workspace(L.gsr_sam_neck_workspace_bytes(g, hid, Cn), dev)
    p = S.VISION + "layers.0."
    out(f" encoder stages, T = {T} tokens, hidden {hid}, {heads} heads of {hd}:")
    sums = {}
    sums["embed"] = attempt(out, "embed (768-GEMM + position)", lambda: chk(L.gsr_sam_embed(
        ptr(x), cfg.image_size, hid, ptr(t[S.VISION + "patch_embed.projection.weight"]), ptr(t[S.VISION + "patch_embed.projection.bias"]),
        ptr(t[S.VISION + "pos_embed"]), ptr(ws_e), ws_e.numel(), ptr(emb), s)), dev, args, 2.0 * T * 768 * hid)
    sums["norm"] = attempt(out, "norm (fp32 -> fp16)", lambda: chk(L.gsr_dino_norm(
        ptr(resid), T, hid, hid, ptr(t[p + "layer_norm1.weight"]), ptr(t[p + "layer_norm1.bias"]), 1e-6, 0, ptr(xn), s)), dev, args)
    sums["qkv"] = attempt(out, f"linear {hid}->{3 * hid} + bias (qkv)", lambda: chk(L.gsr_dino_linear(
        ptr(xn), ptr(t[p + "attn.qkv.weight"]), ptr(t[p + "attn.qkv.bias"]), None, T, hid, 3 * hid, 0, ptr(qkv), s)), dev, args, 6.0 * T * hid * hid)
    for label, layer in (("windowed", win), ("global", glob)):
        if layer is None:
            continue
        wsz = cfg.windows()[layer]
        sz = g if wsz == 0 else wsz
        nw = -(-g // sz)
        pl = f"{S.VISION}layers.{layer}.attn."
        ws_a = workspace(L.gsr_sam_attn_workspace_bytes(g, wsz, heads), dev)
        sums["attn_" + label] = attempt(out, f"attention, {label} (s = {sz}, {nw * nw} windows, bias pre-pass in)", lambda: chk(L.gsr_sam_attn(
            ptr(qkv), ptr(t[pl + "qkv.bias"]), ptr(t[pl + "rel_pos_h"]), ptr(t[pl + "rel_pos_w"]), 2 * sz - 1, g, wsz, heads, hd, ptr(ws_a),
            ws_a.numel(), ptr(att), s)), dev, args, 4.0 * heads * nw * nw * sz ** 4 * hd)
    # the residual and GELU epilogues are timed through the whole encoder only: gsr_dino_linear exposes epilogues 0..2, and
    # LayerScale's (2) costs what the plain residual does
    sums["proj"] = attempt(out, f"linear {hid}->{hid} + bias (as proj)", lambda: chk(L.gsr_dino_linear(
        ptr(att), ptr(t[p + "attn.proj.weight"]), ptr(t[p + "attn.proj.bias"]), None, T, hid, hid, 0, ptr(xn), s)), dev, args, 2.0 * T * hid * hid)
    sums["lin1"] = attempt(out, f"linear {hid}->{mlp} + GELU (lin1)", lambda: chk(L.gsr_dino_linear(
        ptr(xn), ptr(t[p + "mlp.lin1.weight"]), ptr(t[p + "mlp.lin1.bias"]), None, T, hid, mlp, 1, ptr(act), s)), dev, args, 2.0 * T * hid * mlp)
    sums["lin2"] = attempt(out, f"linear {mlp}->{hid} + bias (as lin2)", lambda: chk(L.gsr_dino_linear(
        ptr(act), ptr(t[p + "mlp.lin2.weight"]), ptr(t[p + "mlp.lin2.bias"]), None, T, mlp, hid, 0, ptr(xn), s)), dev, args, 2.0 * T * hid * mlp)
    n = S.VISION + "neck."
    sums["neck"] = attempt(out, "neck (1x1, norm, 3x3, norm)", lambda: chk(L.gsr_sam_neck(
        ptr(resid), g, hid, Cn, ptr(t[n + "conv1.weight"]), ptr(t[n + "layer_norm1.weight"]), ptr(t[n + "layer_norm1.bias"]),
        ptr(t[n + "conv2.weight"]), ptr(t[n + "layer_norm2.weight"]), ptr(t[n + "layer_norm2.bias"]), ptr(ws_n), ws_n.numel(), ptr(feat), s)),
        dev, args, 2.0 * T * Cn * (hid + 9 * Cn))
    # the twin's layers on the same GPU: one windowed and one global SamVisionLayer, fp32 and fp16
    for dtype, label in ((torch.float32, "fp32"), (torch.float16, "fp16")):
        try:
            model = S.host_encoder(w, dtype, dev)
            xs = torch.randn(1, g, g, hid, generator=gen).to(device=dev, dtype=dtype)
            for kind, layer in (("windowed", win), ("global", glob)):
                if layer is not None:
                    attempt(out, f"transformers SamVisionLayer {kind} {label}", lambda: model.layers[layer](xs), dev, args)
            del model
        except Exception as e:
            out(f"  transformers layers {label} failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()


def encoder_flop(cfg):
    g, hid, heads, hd = cfg.grid, cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim
    T = g * g
    total = 2.0 * T * 768 * hid + 2.0 * T * cfg.output_channels * (hid + 9 * cfg.output_channels)
    for wsz in cfg.windows():
        sz = g if wsz == 0 else wsz
        nw = -(-g // sz)
        total += 2.0 * T * (4 * hid * hid + 2 * hid * cfg.mlp_dim) + 4.0 * heads * nw * nw * sz ** 4 * hd
    return total


def whole(cfg, w, dev, args, out):
    x = torch.randn(3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(1)).to(torch.float16).float().to(dev)
    flop = encoder_flop(cfg)
    out(f" whole encoder at {cfg.image_size}x{cfg.image_size} ({flop / 1e12:.2f} TFLOP counted from the shapes, padded window positions included):")
    enc = S.SamImageEncoder(w)
    ours = None
    if attempt(out, "kernels (gsr_sam_encode)", lambda: enc.encode(x), dev, args, flop) is not None:
        ours = enc.encode(x).double()
    for dtype, label in ((torch.float32, "fp32 (the reference's precision)"), (torch.float16, "fp16")):
        try:
            model = S.host_encoder(w, dtype, dev)
            attempt(out, f"transformers SamVisionEncoder {label}", lambda: S.sam_host(w, x, dtype, dev, model), dev, args, flop)
            if ours is not None:
                out(f"  max |kernels - transformers {label.split()[0]}|: {float((S.sam_host(w, x, dtype, dev, model).double() - ours).abs().max()):.3e}")
            del model
        except Exception as e:
            out(f"  transformers {label} failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()


class Sam:
    """What selection, decoder_whole and image read of a model (scripts/sam2_bench.py passes its own)."""
    generator, twin, entry, modules = S.SamMaskGenerator, "decode_host", "gsr_sam_decode", "prompt encoder and mask decoder"
    host_decoder = staticmethod(S.host_decoder)

    @staticmethod
    def embedding(g, dev):
        return torch.randn(1, 256, g, g, generator=torch.Generator().manual_seed(5)).to(torch.float16).float().to(dev)

    @staticmethod
    def frame(size):
        return size - 8, size

    @staticmethod
    def decode_host(w, emb, pts, dtype, dev, modules):
        return S.decode_host(w, emb, None, pts, dtype, dev, modules)


def selection(dev, args, out, points=1024, model=Sam):
    # cones a (r - d) / r plus smooth noise: a in [20, 120] puts about half of them above the stability threshold (the
    # score of a clean cone is ((1 - 1/a) / (1 + 1/a))^2), and predicted ious uniform in [0.5, 1] let 28 % through the first gate
    direct = model.generator.DIRECT          # SAM2: one resampling to the mask's size, input_size is not read
    gen = torch.Generator().manual_seed(2)
    Lr, n = 256, points * 3
    ys, xs = torch.meshgrid(torch.arange(Lr, dtype=torch.float32, device=dev), torch.arange(Lr, dtype=torch.float32, device=dev), indexing="ij")
    rnd = lambda lo, hi: (lo + (hi - lo) * torch.rand(n, generator=gen)).to(dev)[:, None, None]
    a, cy, cx, r = rnd(20.0, 120.0), rnd(0.0, 256.0 if direct else 170.0), rnd(0.0, 256.0), rnd(16.0, 128.0)
    low = torch.empty(n, Lr, Lr, device=dev)
    for k in range(0, n, 256):
        sl = slice(k, k + 256)
        noise = torch.nn.functional.interpolate(torch.randn(a[sl].shape[0], 1, 32, 32, generator=gen).to(dev), (Lr, Lr), mode="bilinear")[:, 0]
        low[sl] = a[sl] * (r[sl] - torch.sqrt((ys - cy[sl]) ** 2 + (xs - cx[sl]) ** 2)) / r[sl] + 0.7 * noise
    low = low.reshape(points, 3, Lr, Lr)
    iou = (0.5 + 0.5 * torch.rand(points, 3, generator=gen)).to(dev)
    stub = model.generator.__new__(model.generator)
    stub.host, stub.pred_iou_thresh, stub.stability_score_thresh, stub.stability_score_offset, stub.box_nms_thresh = False, 0.86, 0.92, 1.0, 0.7
    out(f" {'one-step ' if direct else ''}select: {points} points x 3 masks of {Lr}x{Lr} logits"
        f"{'' if direct else f' ({low.numel() * 4 / 1e6:.0f} MB held)'}, thresholds 0.86 / 0.92 / 0.7:")
    for size in ((768, 1024), (680, 1024)):
        kept, frame = None, None if direct else size
        try:
            kept = len(stub.select(low, iou, frame, size)["index"])
        except Exception as e:
            out(f"  select {size} failed: {type(e).__name__}: {e}")
        attempt(out, f"kernels, masks {size[1]}x{size[0]} ({kept} kept)", lambda: stub.select(low, iou, frame, size), dev, args)
        attempt(out, f"select_host{' direct' if direct else ''} (torch fp32), masks {size[1]}x{size[0]}",
                lambda: S.select_host(low, iou, frame, size, direct=direct), dev, args)
        torch.cuda.empty_cache()


def decoder_stages(cfg, w, dev, args, out, P=256):
    """The stage entry points of csrc/sam_decoder.hip at the grid of `cfg` with P points (random inputs of the right shapes)."""
    L, s, chk = _lib.lib(), stream(dev), _lib.check
    g = cfg.grid
    T = g * g
    gen = torch.Generator().manual_seed(4)
    h16 = lambda *shape: torch.randn(*shape, generator=gen).to(torch.float16).to(dev)
    f32 = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    table = [t.to(dev) for t in w.decoder_table()]
    out(f" decoder stages, g = {g} (T = {T} image tokens), {P} points, 7 tokens per point:")
    pts, sparse = (1024 * torch.rand(P, 2, generator=gen)).to(dev), torch.empty(P, 2, 256, device=dev)
    attempt(out, "prompt (2 sparse tokens per point)", lambda: chk(L.gsr_sam_dec_prompt(
        ptr(pts), P, cfg.image_size, ptr(table[0]), ptr(table[1]), ptr(table[2]), ptr(sparse), s)), dev, args)
    q, kpe, o16 = f32(P, 7, 128), f32(T, 128), torch.empty(P, 7, 128, dtype=torch.float16, device=dev)
    kx, v = h16(P, T, 128), h16(P, T, 128)
    flop = 4.0 * P * 7 * T * 128
    attempt(out, "t2i attention, per-image keys (layer 0)", lambda: chk(L.gsr_sam_dec_t2i(
        ptr(q), ptr(kx), ptr(kpe), ptr(v), P, T, 1, ptr(o16), s)), dev, args, flop)
    attempt(out, "t2i attention, per-point keys (layer 1, final)", lambda: chk(L.gsr_sam_dec_t2i(
        ptr(q), ptr(kx), ptr(kpe), ptr(v), P, T, 0, ptr(o16), s)), dev, args, flop)
    x = h16(P, T, 256)
    attempt(out, "linear 256->128 on the image stream (k, v, q)", lambda: chk(L.gsr_dino_linear(
        ptr(x), ptr(table[_lib.GSR_SAMD_W_LAYER0 + 12]), None, None, P * T, 256, 128, 0, ptr(kx), s)), dev, args, 2.0 * P * T * 256 * 128)
    k7, v7 = f32(P, 7, 128), f32(P, 7, 128)
    it = _lib.GSR_SAMD_W_LAYER0 + 28
    n4 = _lib.GSR_SAMD_W_LAYER0 + 26
    nb = L.gsr_sam_dec_i2t_workspace_bytes(P, T)
    ws = workspace(nb, dev)
    attempt(out, "i2t (attention, out_proj, residual, layer_norm4)", lambda: chk(L.gsr_sam_dec_i2t(
        ptr(kx), ptr(kpe), ptr(k7), ptr(v7), ptr(x), P, T, 0, ptr(table[it + 6]), ptr(table[it + 7]), ptr(table[n4]), ptr(table[n4 + 1]),
        ptr(ws), nb, ptr(x), s)), dev, args, 4.0 * P * T * 7 * 128 + 2.0 * P * T * 128 * 256)
    del ws
    up = _lib.GSR_SAMD_W_UP
    hyper, low = f32(3, P, 32), torch.empty(P, 3, 4 * g, 4 * g, device=dev)
    nb = L.gsr_sam_dec_upscale_workspace_bytes(g, P)
    ws = workspace(nb, dev)
    attempt(out, "upscale (conv1, norm, GELU, conv2, GELU, masks)", lambda: chk(L.gsr_sam_dec_upscale(
        ptr(x), g, P, *[ptr(t) for t in table[up:up + 6]], ptr(hyper), ptr(ws), nb, ptr(low), s)), dev, args,
        2.0 * P * T * (256 * 256 + 4 * 64 * 128 + 16 * 32 * 3))


def decoder_whole(cfg, w, dev, args, out, points=1024, model=Sam):
    """The whole prompt encoder and mask decoder for `points` points: the kernels next to the model's decode_host in fp32 (what
    the generator runs by default) and in fp16 (the strongest stock alternative), on the same GPU in the same run."""
    g, twin, entry = cfg.image_size // 16, model.twin, model.entry
    emb = model.embedding(g, dev)
    pts = S.point_grid(int(round(points ** 0.5)), model.frame(cfg.image_size))
    out(f" whole decoder, g = {g}, {len(pts)} points (decoder='hip' chunks them by {S.DECODER_WORKSPACE_BUDGET >> 20} MiB of workspace; "
        f"{twin} takes 64 at a time):")
    gen = model.generator(w, device=dev, decoder="hip")
    t = {}
    try:
        with torch.no_grad():
            t["hip"] = timed(lambda: gen.decode(emb, pts), dev, args.warmup, args.repeats)
        out(fmt(f"kernels ({entry})", t["hip"]))
        ours = gen.decode(emb, pts)
    except Exception as e:
        out(f"  kernels ({entry}) failed: {type(e).__name__}: {e}")
        ours = None
    for dtype, label in ((torch.float32, "fp32 (the generator's default)"), (torch.float16, "fp16")):
        try:
            modules = model.host_decoder(w, dtype, dev)
            with torch.no_grad():
                t[label[:4]] = timed(lambda: model.decode_host(w, emb, pts, dtype, dev, modules), dev, args.warmup, args.repeats)
            out(fmt(f"{twin} {label}", t[label[:4]]))
            if ours is not None:
                lo, io = model.decode_host(w, emb, pts, dtype, dev, modules)
                out(f"  max |kernels - {twin} {label[:4]}|: masks {float((lo.float() - ours[0]).abs().max()):.3e}, "
                    f"iou {float((io.float() - ours[1]).abs().max()):.3e}")
            del modules
        except Exception as e:
            out(f"  {twin} {label} failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()
    if "hip" in t and "fp16" in t:
        margin = t["fp16"][0] - t["hip"][0]
        spread = max(t["hip"][2] - t["hip"][1], t["fp16"][2] - t["fp16"][1])
        verdict = "below" if margin > spread else "NOT below"
        out(f"  kernels {verdict} {twin} fp16: margin {margin:.3f} ms against a spread of {spread:.3f} ms (the larger min..max)")
    if "hip" in t and "fp32" in t:
        out(f"  kernels {'below' if t['hip'][0] < t['fp32'][0] else 'NOT below'} {twin} fp32: {t['fp32'][0] / t['hip'][0]:.2f} x")


def image(cfg, w, dev, args, out, decoder="torch", model=Sam):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 255, (768, 1024, 3), dtype=np.uint8)
    gen = model.generator(w, points_per_side=args.points_per_side, device=dev, decoder=decoder)
    rows = []
    for _ in range(args.warmup + 3):
        gen.generate_device(img)
        rows.append(dict(gen.last_ms))
    last = rows[-1]
    total = sum(last.values())
    out(f" one 1024x768 image, {args.points_per_side ** 2} points, decoder={decoder!r} (host preprocessing inside embed; the last of {len(rows)} runs):")
    for k in ("embed", "decode", "select"):
        out(f"  {k:<52s} {last[k]:9.3f} ms  ({100 * last[k] / total:.1f} % of the image)")
    if decoder == "torch":
        out(f"  decode is transformers' {model.modules} in fp32 torch, as they are")
    else:
        out(f"  decode is {model.entry}: the kernels of csrc/sam_decoder.hip")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_bench.txt"))
    ap.add_argument("--model_type", default="vit_h")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points_per_side", type=int, default=32)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sam_bench: no HIP device; timings are taken on the GPU only")
    dev = torch.device("cuda", 0)
    _lib.lib()
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a later section that dies does not lose the earlier ones
            f.write("\n".join(lines) + "\n")
    cfg = S.SamConfig.preset(args.model_type)
    w = S.random_sam_weights(cfg, seed=0)
    import transformers
    out(f"SAM {args.model_type} ({cfg.num_hidden_layers} layers, hidden {cfg.hidden_size}, window {cfg.window_size}, random weights) on "
        f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}, transformers {transformers.__version__}")
    out(f"median of {args.repeats} timed calls after {args.warmup} warm-up calls, (min .. max); TFLOP/s = operations counted from the shapes / median")
    for section in (stages, whole):
        try:
            section(cfg, w, dev, args, out)
        except Exception as e:
            out(f" {section.__name__} failed: {type(e).__name__}: {e}")
    try:
        selection(dev, args, out)
    except Exception as e:
        out(f" selection failed: {type(e).__name__}: {e}")
    for section in (decoder_stages, decoder_whole):
        try:
            section(cfg, w, dev, args, out)
        except Exception as e:
            out(f" {section.__name__} failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()
    for decoder in ("torch", "hip"):
        try:
            image(cfg, w, dev, args, out, decoder)
        except Exception as e:
            out(f" image ({decoder}) failed: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
