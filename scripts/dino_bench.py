"""Time the DINOv3 ViT encoder on one GPU: the kernels of csrc/dino.hip and csrc/vit.hip stage by stage and as a whole, transformers' fp16
model with its default attention on the same GPU next to it, and the training step with the feature term off, on a side
stream and on the training stream.

    python scripts/dino_bench.py [--out profiles/dino_bench.txt] [--sizes 1600x1200,1920x1080] [--points 200000] [--steps 40]

Random ViT-B/16 weights (gaussmart_amd.dino.random_dino_weights) and seeded images: nothing outside the repository is read.
Every figure is the median of `--repeats` timed calls (device events around one call each, after `--warmup` untimed calls of
the same shape); the spread (min .. max) is printed beside it.  TFLOP/s are the useful operations counted from the shapes
(2 M K N per product, 4 T^2 64 per head for attention) over that time: a rate the call reached, not a share of peak.  These
figures are reported, not gated: stages slower than torch's stay in the table."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                 # noqa: E402

from gaussmart_amd import _lib, dino as D                    # noqa: E402
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
    return f"  {name:<44s} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f}){rate}"


def stages(cfg, w, B, H, W, dev, args, out):
    L = _lib.lib()
    s = stream(dev)
    hid, inter, heads = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
    Hp, Wp = H // 16, W // 16
    T = cfg.tokens(H, W)
    M = B * T
    g = torch.Generator().manual_seed(0)
    h16 = lambda *shape: torch.randn(*shape, generator=g).to(torch.float16).to(dev)
    x = torch.rand(B, 3, H, W, generator=g).to(dev)
    resid = torch.randn(M, hid, generator=g).to(dev)
    xn, q, k, v, att, mlp = h16(M, hid), h16(M, hid), h16(M, hid), h16(M, hid), h16(M, hid), h16(M, inter)
    wd = w.to(dev)
    t = wd.tensors
    p0 = wd.prefix + ".0."
    c = cfg.to_c()
    import ctypes as C
    nb = L.gsr_dino_embed_workspace_bytes(B, H, W)
    ws = workspace(nb, dev)
    emb = torch.empty(M, hid, device=dev)
    chk = _lib.check
    run = {
        "embed (normalise + 768-GEMM)": (lambda: chk(L.gsr_dino_embed(C.byref(c), ptr(x), None, B, H, W, ptr(t["embeddings.cls_token"]),
                                                                       ptr(t["embeddings.register_tokens"]), ptr(t["embeddings.patch_embeddings.weight"]),
                                                                       ptr(t["embeddings.patch_embeddings.bias"]), ptr(ws), nb, ptr(emb), s)),
                                         2.0 * B * Hp * Wp * 768 * hid),
        "norm (fp32 -> fp16)": (lambda: chk(L.gsr_dino_norm(ptr(resid), M, hid, hid, ptr(t[p0 + "norm1.weight"]), ptr(t[p0 + "norm1.bias"]), 1e-5, 0,
                                                            ptr(xn), s)), None),
        f"linear {hid}->{hid} + bias (q, k, v each)": (lambda: chk(L.gsr_dino_linear(ptr(xn), ptr(t[p0 + "attention.q_proj.weight"]),
                                                                                      ptr(t[p0 + "attention.q_proj.bias"]), None, M, hid, hid, 0, ptr(q), s)),
                                                       2.0 * M * hid * hid),
        "rope (q and k)": (lambda: chk(L.gsr_dino_rope(ptr(q), ptr(k), B, T, heads, Hp, Wp, 100.0, s)), None),
        "attention": (lambda: chk(L.gsr_dino_attn(ptr(q), ptr(k), ptr(v), B, T, heads, ptr(att), s)), 4.0 * B * heads * T * T * 64),
        f"linear {hid}->{hid} + LayerScale + residual": (lambda: chk(L.gsr_dino_linear(ptr(att), ptr(t[p0 + "attention.o_proj.weight"]),
                                                                                        ptr(t[p0 + "attention.o_proj.bias"]), ptr(t[p0 + "layer_scale1.lambda1"]),
                                                                                        M, hid, hid, 2, ptr(resid), s)), 2.0 * M * hid * hid),
        f"linear {hid}->{inter} + GELU": (lambda: chk(L.gsr_dino_linear(ptr(xn), ptr(t[p0 + "mlp.up_proj.weight"]), ptr(t[p0 + "mlp.up_proj.bias"]), None,
                                                                         M, hid, inter, 1, ptr(mlp), s)), 2.0 * M * hid * inter),
        f"linear {inter}->{hid} + LayerScale + residual": (lambda: chk(L.gsr_dino_linear(ptr(mlp), ptr(t[p0 + "mlp.down_proj.weight"]),
                                                                                          ptr(t[p0 + "mlp.down_proj.bias"]), ptr(t[p0 + "layer_scale2.lambda1"]),
                                                                                          M, inter, hid, 2, ptr(resid), s)), 2.0 * M * hid * inter),
    }
    # the torch side of the same stages, fp16 on the same device (rocBLAS / torch's default scaled_dot_product_attention)
    F = torch.nn.functional
    q4 = lambda a: a.view(B, T, heads, 64).transpose(1, 2)
    wq, bq = t[p0 + "attention.q_proj.weight"], t[p0 + "attention.q_proj.bias"]
    wu, bu, wdn, bdn = t[p0 + "mlp.up_proj.weight"], t[p0 + "mlp.up_proj.bias"], t[p0 + "mlp.down_proj.weight"], t[p0 + "mlp.down_proj.bias"]
    torch_run = {
        f"torch F.linear {hid}->{hid} fp16": (lambda: F.linear(xn, wq, bq), 2.0 * M * hid * hid),
        f"torch F.linear {hid}->{inter} + gelu fp16": (lambda: F.gelu(F.linear(xn, wu, bu)), 2.0 * M * hid * inter),
        f"torch F.linear {inter}->{hid} fp16": (lambda: F.linear(mlp, wdn, bdn), 2.0 * M * hid * inter),
        "torch scaled_dot_product_attention fp16": (lambda: F.scaled_dot_product_attention(q4(q), q4(k), q4(v)), 4.0 * B * heads * T * T * 64),
    }
    out(f" stages, B = {B}, T = {T} tokens per image:")
    for table in (run, torch_run):
        for name, (fn, flop) in table.items():
            try:
                with torch.no_grad():
                    out(fmt(name, timed(fn, dev, args.warmup, args.repeats), flop))
            except Exception as e:          # one stage that fails must not lose the others
                out(f"  {name:<44s} failed: {type(e).__name__}: {e}")


def model_flop(cfg, B, H, W):
    T, hid, inter = cfg.tokens(H, W), cfg.hidden_size, cfg.intermediate_size
    per_layer = 2.0 * T * (4 * hid * hid + 2 * hid * inter) + 4.0 * cfg.num_attention_heads * T * T * 64
    return B * (cfg.num_hidden_layers * per_layer + 2.0 * (H // 16) * (W // 16) * 768 * hid)


def whole(cfg, w, H, W, dev, args, out):
    enc = D.DINOImageEncoder(w)
    g = torch.Generator().manual_seed(1)
    for B in (1, 2):
        x = torch.rand(B, 3, H, W, generator=g).to(dev)
        flop = model_flop(cfg, B, H, W)
        out(f" whole encoder, B = {B} ({flop / 1e12:.2f} TFLOP counted from the shapes):")
        pooled = None
        try:
            out(fmt("kernels (gsr_dino_forward)", timed(lambda: enc.forward(x), dev, args.warmup, args.repeats), flop))
            pooled = enc.forward(x)[0].double()
        except Exception as e:
            out(f"  kernels failed: {type(e).__name__}: {e}")
        try:
            model = D.host_model(w, torch.float16, dev)
            attn = getattr(model.config, "_attn_implementation", "?")
            mean = torch.tensor(cfg.image_mean, device=dev, dtype=torch.float16).view(1, 3, 1, 1)
            std = torch.tensor(cfg.image_std, device=dev, dtype=torch.float16).view(1, 3, 1, 1)

            def hf():
                with torch.inference_mode():
                    return model((x.half() - mean) / std).pooler_output
            out(fmt(f"transformers fp16 (attention: {attn})", timed(hf, dev, args.warmup, args.repeats), flop))
            if pooled is not None:
                out(f"  max |kernels - transformers fp16| over the pooled rows: {float((hf().double() - pooled).abs().max()):.3e}")
            del model
        except Exception as e:
            out(f"  transformers fp16 failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()


def training(cfg, w, H, W, dev, args, out):
    from gaussmart_amd.gaussian_model import GaussianModel
    from gaussmart_amd.gaussian_renderer import render
    from gaussmart_amd.params import OptimizationParams, PipelineParams
    from gaussmart_amd.synthetic import make_scene, jittered_cameras, perturb
    from gaussmart_amd.trainer import train, DinoTerm, TrainState
    params, _ = make_scene(args.points, W, H, seed=0)
    cams = jittered_cameras(4, W, H, seed=0, device=dev, amount=0.1)
    bg = torch.zeros(3, device=dev)
    pipe, opt = PipelineParams(), OptimizationParams()
    opt.densify_until_iter = 0
    target = GaussianModel(3, device=dev)
    target.create_from_params(perturb(params))
    with torch.no_grad():
        for cam in cams:
            cam.original_image = render(cam, target, pipe, bg, surface_maps=False)["render"].clamp(0, 1)
    out(f" training step at {W}x{H}, {args.points} surfels, {args.steps} iterations per figure (after {args.steps // 4} untimed ones):")
    for label, make in (("term off", lambda: None),
                        ("term on, side stream", lambda: DinoTerm(D.DINOImageEncoder(w), 0.05, 0, side_stream=True)),
                        ("term on, training stream", lambda: DinoTerm(D.DINOImageEncoder(w), 0.05, 0, side_stream=False))):
        try:
            model = GaussianModel(3, device=dev)
            model.create_from_params(params)
            model.training_setup(opt)
            term, state = make(), TrainState(0)
            n0 = args.steps // 4
            train(model, cams, opt, pipe, bg, first_iter=8000, iterations=8000 + n0, final_iteration=30000, state=state, dino=term)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            train(model, cams, opt, pipe, bg, first_iter=8000 + n0, iterations=8000 + n0 + args.steps, final_iteration=30000, state=state, dino=term)
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) / args.steps * 1e3
            extra = ""
            if term is not None:
                rows = term.rows()
                extra = f"   (last logged dino_loss {rows[-1][1]:.5f}, total {rows[-1][2]:.5f})"
            out(f"  {label:<44s} {dt:9.3f} ms / iteration{extra}")
        except Exception as e:
            out(f"  {label:<44s} failed: {type(e).__name__}: {e}")
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_bench.txt"))
    ap.add_argument("--sizes", default="1600x1200,1920x1080")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--layers", type=int, default=12)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dino_bench: no HIP device; timings are taken on the GPU only")
    dev = torch.device("cuda", 0)
    _lib.lib()
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)
    cfg = D.DinoConfig(num_hidden_layers=args.layers)
    w = D.random_dino_weights(cfg, seed=0)
    import transformers
    out(f"DINOv3 ViT-B/16 encoder ({cfg.num_hidden_layers} layers, hidden {cfg.hidden_size}, random weights) on {torch.cuda.get_device_name(0)}; "
        f"torch {torch.__version__}, transformers {transformers.__version__}")
    out(f"median of {args.repeats} timed calls after {args.warmup} warm-up calls, (min .. max); TFLOP/s = operations counted from the shapes / median")
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.lower().split("x"))
        out(f"\n{W}x{H}:")
        stages(cfg, w, 1, H, W, dev, args, out)
        whole(cfg, w, H, W, dev, args, out)
        try:
            training(cfg, w, H, W, dev, args, out)
        except Exception as e:
            out(f" training step failed: {type(e).__name__}: {e}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
