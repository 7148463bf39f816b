"""Time SAM2 mask generation on one GPU: the Hiera encoder and FPN neck of csrc/sam2.hip, whole and stage by stage at 1024x1024,
next to transformers' Sam2Model.get_image_embeddings in fp32 (the reference's precision) and in fp16 on the same GPU; HV_ATTN
per block kind of Hiera-large (8x8, 4x4 and 16x16 windows, the three pooled stage starts, the global block over 4096 keys);
the one-step mask selection next to its torch twin; the decoder kernels of csrc/sam_decoder.hip with SAM2's eight tokens and
two skips, stage by stage and as a whole for 1024 points, next to decode_host2 in fp32 and in fp16; and an image's time split
into embed / decode / select with either decoder.

    python scripts/sam2_bench.py [--out profiles/sam2_bench.txt] [--model_type large] [--points_per_side 32] [--ab_lib FILE]

--ab_lib: a second build of the library with feat_s0 added by a kernel of its own instead of conv2's epilogue (`make -C
gaussmart_amd/csrc BUILD=build_ab OUT=../lib_ab/libgsr_hip.so EXTRA_DEFS=-DSD_SKIP0_EPILOGUE=0`); its up-scaling is timed in
alternation with the product's, in the same process.

Random weights (gaussmart_amd.sam2.random_sam2_weights) and seeded inputs: nothing outside the repository is read.  Every
figure is the median of `--repeats` timed calls (device events around one call each, after `--warmup` untimed calls of the
same shape); the spread (min .. max) is printed beside it.  The kernels' per-stage times are taken through the stage entry
points (the same launches gsr_sam2_encode makes, issued from Python), transformers' by running its blocks stage by stage.  These
figures are reported, not gated: entries slower than torch's stay in the table."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch                                                 # noqa: E402

from sam_bench import attempt, decoder_whole, image, selection         # noqa: E402
from gaussmart_amd import _lib, sam2 as S2                   # noqa: E402
from gaussmart_amd._dev import ptr, stream, workspace       # noqa: E402


def encoder_flop(cfg):
    """Useful operations of the encoder counted from the shapes, per stage (the neck with the last)."""
    dims, grids, heads = cfg.dims(), cfg.grids(), cfg.heads()
    per = [2.0 * grids[0] ** 2 * S2.PATCH_K * dims[0], 0.0, 0.0, 0.0]
    for i, start, g, win, stride in cfg.block_plan():
        d, T_in, T = dims[i], g * g, (g // stride) ** 2
        d_in = d // 2 if start else d
        s = win or g
        f = 2.0 * T_in * d_in * 3 * d + (2.0 * T_in * d_in * d if start else 0.0)       # qkv, the stage start's projection
        f += 4.0 * T * s * s * d                                                        # scores and P V, all heads
        f += 2.0 * T * d * d + 16.0 * T * d * d                                         # attn.proj, the MLP
        per[i] += f
    D = cfg.fpn_hidden_size
    per[3] += sum(2.0 * grids[i] ** 2 * dims[i] * D for i in range(4)) + 2.0 * D * (grids[0] ** 2 * D // 8 + grids[1] ** 2 * D // 4)
    return per


class StageRunner:
    """The launches of gsr_sam2_encode, stage by stage, through the stage entry points (for the per-stage times only)."""

    def __init__(self, w, dev):
        self.cfg, self.dev = w.config, dev
        self.tab = w.to(dev).table()
        cfg, g0, d0 = self.cfg, w.config.image_size // 4, w.config.embed_dim
        row = g0 * g0 * d0
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        f16 = lambda n: torch.empty(n, dtype=torch.float16, device=dev)
        self.resid, self.proj, self.xn, self.qkv, self.att, self.mlp = [f32(row), f32(row)], f32(2 * row), f16(row), f16(6 * row), f16(row), f16(4 * row)
        self.ws_e = workspace(_lib.lib().gsr_sam2_embed_workspace_bytes(cfg.image_size), dev)
        self.ws_n = workspace(_lib.lib().gsr_sam2_neck_workspace_bytes(g0, d0, cfg.fpn_hidden_size), dev)
        D, g = cfg.fpn_hidden_size, cfg.grids()
        self.outs = [torch.empty(c, gi, gi, device=dev) for c, gi in ((D // 8, g[0]), (D // 4, g[1]), (D, g[2]))]
        self.ends = [f32(g[i] * g[i] * (d0 << i)) for i in range(4)]
        self.cur = 0

    def stage(self, i, x=None):
        L, s, chk, cfg, t = _lib.lib(), stream(self.dev), _lib.check, self.cfg, self.tab
        lin = lambda a, w, b, M, K, N, epi, out: chk(L.gsr_sam2_linear(ptr(a), ptr(w), ptr(b), None, M, K, N, epi, ptr(out), s))
        norm = lambda a, rows, d, w, b, out: chk(L.gsr_dino_norm(ptr(a), rows, d, d, ptr(w), ptr(b), 1e-6, 0, ptr(out), s))
        if i == 0:
            self.cur = 0
            chk(L.gsr_sam2_embed(ptr(x), cfg.image_size, cfg.embed_dim, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(self.ws_e), self.ws_e.numel(),
                                 ptr(self.resid[0]), s))
        for k, (st, start, g, win, stride) in enumerate(cfg.block_plan()):
            if st != i:
                continue
            b = t[3 + 14 * k:3 + 14 * (k + 1)]
            d, heads = cfg.dims()[st], cfg.heads()[st]
            T_in, T, d_in = g * g, (g // stride) ** 2, (d // 2 if start else d)
            norm(self.resid[self.cur], T_in, d_in, b[0], b[1], self.xn)
            if start:
                lin(self.xn, b[12], b[13], T_in, d_in, d, _lib.GSR_SAM2_EPI_F32, self.proj)
                chk(L.gsr_sam2_pool(ptr(self.proj), g, d, ptr(self.resid[self.cur ^ 1]), s))
                self.cur ^= 1
            lin(self.xn, b[2], b[3], T_in, d_in, 3 * d, _lib.GSR_DINO_EPI_BIAS, self.qkv)
            chk(L.gsr_sam2_attn(ptr(self.qkv), g, win, stride, heads, d // heads, ptr(self.att), s))
            r = self.resid[self.cur]
            lin(self.att, b[4], b[5], T, d, d, _lib.GSR_SAM2_EPI_RESID1, r)
            norm(r, T, d, b[6], b[7], self.xn)
            lin(self.xn, b[8], b[9], T, d, 4 * d, _lib.GSR_DINO_EPI_GELU, self.mlp)
            lin(self.mlp, b[10], b[11], T, 4 * d, d, _lib.GSR_SAM2_EPI_RESID1, r)
        n = self.ends[i].numel()
        self.ends[i].copy_(self.resid[self.cur][:n])

    def neck(self):
        cfg = self.cfg
        streams = (C.c_void_p * 4)(*[e.data_ptr() for e in self.ends])
        table = (C.c_void_p * 13)(*[x.data_ptr() for x in self.tab[-13:]])
        _lib.check(_lib.lib().gsr_sam2_neck(streams, cfg.image_size // 4, cfg.embed_dim, cfg.fpn_hidden_size,
                                            sum(1 << l for l in set(cfg.fpn_top_down_levels)), table, ptr(self.ws_n), self.ws_n.numel(),
                                            ptr(self.outs[0]), ptr(self.outs[1]), ptr(self.outs[2]), stream(self.dev)))


def encoder(cfg, w, dev, args, out):
    x = torch.randn(3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(1)).to(torch.float16).float().to(dev)
    per = encoder_flop(cfg)
    flop = sum(per)
    out(f" whole encoder at {cfg.image_size}x{cfg.image_size} ({flop / 1e12:.2f} TFLOP counted from the shapes):")
    enc = S2.Sam2ImageEncoder(w)
    ours = None
    if attempt(out, "kernels (gsr_sam2_encode)", lambda: enc.encode(x), dev, args, flop) is not None:
        ours = [m.double() for m in enc.encode(x)]
    models = {}
    for dtype, label in ((torch.float32, "fp32 (the reference's precision)"), (torch.float16, "fp16")):
        try:
            models[dtype] = model = S2.host_model(w, dtype, dev)
            attempt(out, f"transformers get_image_embeddings {label}", lambda: S2.sam2_host(w, x, dtype, dev, model), dev, args, flop)
            if ours is not None:
                theirs = S2.sam2_host(w, x, dtype, dev, model)
                out("  max |kernels - transformers " + label.split()[0] + "| per map: " + ", ".join(f"{float((a.double() - b).abs().max()):.3e}" for a, b in zip(theirs, ours)))
        except Exception as e:
            out(f"  transformers {label} failed: {type(e).__name__}: {e}")
    out(f" per stage (blocks {tuple(cfg.blocks_per_stage)}, widths {cfg.dims()}, grids {cfg.grids()}; stage 0 with the patch embedding):")
    run = StageRunner(w, dev)
    with torch.no_grad():
        for i in range(4):
            for k in range(i):                      # the stream this stage starts from
                run.stage(k, x)
            cur = run.cur
            saved = run.resid[cur].clone()

            def one(i=i, cur=cur, saved=saved):
                run.cur = cur
                run.resid[cur].copy_(saved)
                run.stage(i, x)
            attempt(out, f"kernels stage {i} (one stream copy in)", one, dev, args, per[i])
        attempt(out, "kernels neck (laterals, top-down, conv_s0 / conv_s1)", run.neck, dev, args)
        for dtype, model in models.items():
            label = "fp32" if dtype == torch.float32 else "fp16"
            bb = model.vision_encoder.backbone
            h = bb.patch_embed(x[None].to(dtype))
            h = h + bb._get_pos_embed(h.shape[1:3])
            k = 0
            for i, n in enumerate(cfg.blocks_per_stage):
                blocks = bb.blocks[k:k + n]
                k += n

                def one(h=h, blocks=blocks, first=(i == 0)):
                    y = h
                    if first:
                        y = bb.patch_embed(x[None].to(dtype))
                        y = y + bb._get_pos_embed(y.shape[1:3])
                    for b in blocks:
                        y = b(y)
                    return y
                attempt(out, f"transformers stage {i} {label}", one, dev, args, per[i])
                h = one()
    models.clear()
    torch.cuda.empty_cache()


def attention(cfg, dev, args, out):
    kinds = (("8x8 windows, stage 0", 256, 8, 1, 2), ("4x4 windows, stage 1", 128, 4, 1, 4), ("16x16 windows, stage 2", 64, 16, 1, 8),
             ("8x8 windows, stage 3", 32, 8, 1, 16), ("pooled 8x8 -> 4x4, start of stage 1", 256, 8, 2, 4),
             ("pooled 4x4 -> 2x2, start of stage 2", 128, 4, 2, 8), ("pooled 16x16 -> 8x8, start of stage 3", 64, 16, 2, 16),
             ("global, 4096 keys, stage 2", 64, 0, 1, 8))
    hd = cfg.head_dim
    out(f" HV_ATTN per block kind of Hiera-large (head_dim {hd}; TFLOP/s over the scores and P V of the real head width):")
    gen = torch.Generator().manual_seed(3)
    for name, g, w, stride, heads in kinds:
        qkv = torch.randn(g * g, 3 * heads * hd, generator=gen).to(torch.float16).to(dev)
        o = torch.empty((g // stride) ** 2, heads * hd, dtype=torch.float16, device=dev)
        s = w or g
        attempt(out, f"{name} (grid {g}, {heads} heads)", lambda: _lib.check(_lib.lib().gsr_sam2_attn(
            ptr(qkv), g, w, stride, heads, hd, ptr(o), stream(dev))), dev, args, 4.0 * (g // stride) ** 2 * s * s * heads * hd)


class Sam2:
    """sam_bench.Sam for SAM2: what the shared sections (selection, decoder_whole, image) read of the model."""
    generator, twin, entry, modules = S2.Sam2MaskGenerator, "decode_host2", "gsr_sam2_decode", "Sam2PromptEncoder and Sam2MaskDecoder"
    host_decoder, decode_host = staticmethod(S2.host_decoder2), staticmethod(S2.decode_host2)

    @staticmethod
    def embedding(g, dev):
        gen = torch.Generator().manual_seed(5)
        return [torch.randn(shape, generator=gen).to(torch.float16).float().to(dev) for shape in ((32, 4 * g, 4 * g), (64, 2 * g, 2 * g), (256, g, g))]

    @staticmethod
    def frame(size):
        return size, size


CHUNK = 256         # points per call of the stage entry points: about what sam.DECODER_WORKSPACE_BUDGET gives the whole decoder at g = 64


def decoder_stages(cfg, w, dev, args, out, points=1024):
    """The stage entry points of csrc/sam_decoder.hip with SAM2's eight tokens at the grid of `cfg` (random inputs of the right
    shapes).  Every entry is the time of `points` points in calls of CHUNK, as often as one decode runs that stage."""
    L, s, chk = _lib.lib(), stream(dev), _lib.check
    g = cfg.image_size // 16
    T, P, calls = g * g, CHUNK, points // CHUNK
    gen = torch.Generator().manual_seed(4)
    h16 = lambda *shape: torch.randn(*shape, generator=gen).to(torch.float16).to(dev)
    f32 = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    table = [t.to(dev) for t in w.decoder_table()]
    out(f" decoder stages, g = {g} (T = {T} image tokens), {points} points in {calls} calls of {P}, 8 tokens per point; per decode:")
    total = []

    def entry(name, fn, n, flop=None):
        """n calls of fn, timed as one"""
        def run():
            for _ in range(n):
                fn()
        total.append(attempt(out, name, run, dev, args, None if flop is None else flop * n))
    q, kpe, o16 = f32(P, 8, 128), f32(T, 128), torch.empty(P, 8, 128, dtype=torch.float16, device=dev)
    kx, v = h16(P, T, 128), h16(P, T, 128)
    flop = 4.0 * P * 8 * T * 128
    entry("t2i attention, per-image keys (layer 0), x 1", lambda: chk(L.gsr_sam2_dec_t2i(
        ptr(q), ptr(kx), ptr(kpe), ptr(v), P, T, 1, ptr(o16), s)), calls, flop)
    entry("t2i attention, per-point keys (layer 1, final), x 2", lambda: chk(L.gsr_sam2_dec_t2i(
        ptr(q), ptr(kx), ptr(kpe), ptr(v), P, T, 0, ptr(o16), s)), 2 * calls, flop)
    x, xo = h16(P, T, 256), torch.empty(P, T, 256, dtype=torch.float16, device=dev)
    entry("image-stream products 256->128 (k, v, q), x 5", lambda: chk(L.gsr_dino_linear(
        ptr(x), ptr(table[_lib.GSR_SAMD_W_LAYER0 + 12]), None, None, P * T, 256, 128, 0, ptr(kx), s)), 5 * calls, 2.0 * P * T * 256 * 128)
    k8, v8 = f32(P, 8, 128), f32(P, 8, 128)
    it, n4 = _lib.GSR_SAMD_W_LAYER0 + 28, _lib.GSR_SAMD_W_LAYER0 + 26
    nb = L.gsr_sam2_dec_i2t_workspace_bytes(P, T)
    ws = workspace(nb, dev)
    flop = 4.0 * P * T * 8 * 128 + 2.0 * P * T * 128 * 256
    for shared, name in ((1, "per-image stream (layer 0)"), (0, "per-point stream (layer 1)")):
        entry(f"i2t, {name}, x 1", lambda shared=shared: chk(L.gsr_sam2_dec_i2t(
            ptr(kx), ptr(kpe), ptr(k8), ptr(v8), ptr(x), P, T, shared, ptr(table[it + 6]), ptr(table[it + 7]), ptr(table[n4]),
            ptr(table[n4 + 1]), 1e-5, ptr(ws), nb, ptr(xo), s)), calls, flop)
    del ws
    up = _lib.GSR_SAMD_W_UP
    hyper, low = f32(3, P, 32), torch.empty(P, 3, 4 * g, 4 * g, device=dev)
    s0, s1 = f32(32, 4 * g, 4 * g), f32(64, 2 * g, 2 * g)
    flop = 2.0 * P * T * (256 * 256 + 4 * 64 * 128 + 16 * 32 * 3)

    def upscale(lib):
        nb = lib.gsr_sam2_dec_upscale_workspace_bytes(g, P)
        ws = workspace(nb, dev)
        return lambda: chk(lib.gsr_sam2_dec_upscale(ptr(x), g, P, *[ptr(t) for t in table[up:up + 6]], ptr(hyper), ptr(s0), ptr(s1), ptr(ws), nb,
                                                    ptr(low), s)), ws
    fn, ws = upscale(L)
    entry("upscale (conv1 + s1, norm, GELU, conv2 + s0, GELU, masks), x 1", fn, calls, flop)
    rows, hid = h16(points, 256), torch.empty(points, 256, dtype=torch.float16, device=dev)
    hw, hb = table[_lib.GSR_SAMD_W_HYPER], table[_lib.GSR_SAMD_W_HYPER + 1]
    entry("heads (4 MLPs: 12 products on [points,256]; no ReLU pass)", lambda: [chk(L.gsr_dino_linear(
        ptr(rows), ptr(hw), ptr(hb), None, points, 256, 256, 0, ptr(hid), s)) for _ in range(12)], 1)
    if all(t is not None for t in total):
        out(f"  {'sum of the stages above':<52s} {sum(total):9.3f} ms")
    if args.ab_lib:
        B = C.CDLL(args.ab_lib)
        for name in ("gsr_sam2_dec_upscale", "gsr_sam2_dec_upscale_workspace_bytes"):
            getattr(B, name).restype, getattr(B, name).argtypes = getattr(L, name).restype, getattr(L, name).argtypes
        fn_b, ws_b = upscale(B)
        fn()
        ref = low.clone()
        fn_b()
        out(f" feat_s0 in conv2's epilogue (A, the product) or by a kernel of its own on conv2 stored as fp32 (B): {P} points per call, "
            f"alternated; the same bits: {bool(torch.equal(ref, low))}")
        for rnd in range(3):
            attempt(out, f"A upscale, round {rnd}", fn, dev, args, flop)
            attempt(out, f"B upscale, round {rnd}", fn_b, dev, args, flop)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam2_bench.txt"))
    ap.add_argument("--model_type", default="large")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points_per_side", type=int, default=32)
    ap.add_argument("--ab_lib", default=None, help="a -DSD_SKIP0_EPILOGUE=0 build of the library, for the up-scaling's A/B entry")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sam2_bench: no HIP device; timings are taken on the GPU only")
    dev = torch.device("cuda", 0)
    _lib.lib()
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:          # kept current: a later section that dies does not lose the earlier ones
            f.write("\n".join(lines) + "\n")
    cfg = S2.Sam2Config.preset(args.model_type)
    w = S2.random_sam2_weights(cfg, seed=0)
    import transformers
    out(f"SAM2 hiera-{args.model_type} (blocks {tuple(cfg.blocks_per_stage)}, embed {cfg.embed_dim}, windows {tuple(cfg.window_size_per_stage)}, random "
        f"weights) on {torch.cuda.get_device_name(0)}; torch {torch.__version__}, transformers {transformers.__version__}")
    out(f"median of {args.repeats} timed calls after {args.warmup} warm-up calls, (min .. max); TFLOP/s = operations counted from the shapes / median")
    for name, section in (("encoder", lambda: encoder(cfg, w, dev, args, out)), ("attention", lambda: attention(cfg, dev, args, out)),
                          ("selection", lambda: selection(dev, args, out, model=Sam2)),
                          ("decoder stages", lambda: decoder_stages(cfg, w, dev, args, out)),
                          ("decoder", lambda: decoder_whole(cfg, w, dev, args, out, model=Sam2)),
                          ("image (torch)", lambda: image(cfg, w, dev, args, out, "torch", Sam2)),
                          ("image (hip)", lambda: image(cfg, w, dev, args, out, "hip", Sam2))):
        try:
            section()
        except Exception as e:
            out(f" {name} failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
