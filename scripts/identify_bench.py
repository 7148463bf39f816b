"""Times the view selection (step 1 of gaussmart_amd.identify_cli) and every step of the command, on one box:

    python scripts/identify_bench.py [--out profiles/identify_bench.txt] [--model_type vit_b] [--repeats 7]

Step 1 at N = 49, 300 and 1000 cameras (jittered domes): camera_select.select_representative_cameras on the device (all
10 (max_k - 2) fits in one launch of gsr_cam_lloyd), on its numpy twin, and the same decisions through scikit-learn's KMeans
where it imports (130 fits and the reference's refit, as identification/clustering_cameras.py runs them).  The parts of the
device route are timed as well: drawing the k-means++ centres on the host, the launch with its copies, the scores.
Then the whole command on a synthetic dtu scan (49 cameras, 1024x768 pictures, 100 000 points, random SAM weights, --clean,
decoder hip): the time of each step as the command prints it.  Nothing outside the repository is read.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dome_views(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v[:, 2] = np.abs(v[:, 2]) + 0.1
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    pos = v * (3.0 + 0.3 * rng.normal(size=(n, 1)))
    views = {}
    for i, p in enumerate(pos):
        z = -p / np.linalg.norm(p)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, p
        views[i] = {"world_mat": np.linalg.inv(c2w), "scale_mat": np.eye(4),
                    "camera_mat": np.array([[900.0, 0, 512, 0], [0, 900.0, 384, 0], [0, 0, 1, 0], [0, 0, 0, 1]])}
    return views


def timed(fn, warmup, repeats, sync=None):
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(repeats):
        if sync:
            sync()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms), out


def sklearn_select(views):
    """The reference's decisions with scikit-learn's KMeans doing the fits: its 13 x 10 fits and the refit."""
    from sklearn.cluster import KMeans
    from gaussmart_amd import camera_select as CS

    def many(X, ks, **kw):
        out = {}
        for k in ks:
            km = KMeans(n_clusters=k, n_init=10, random_state=42)
            labels = km.fit_predict(X)
            out[k] = (labels.astype(np.int64), km.cluster_centers_, float(km.inertia_))
        return out
    saved = CS.kmeans_many
    CS.kmeans_many = many
    try:
        details = {}
        res = CS.select_representative_cameras(views, details=details)
        many(CS.normalize_positions(CS.camera_centres_dirs(views)[0])[0], [details["best_k"]])        # the reference's refit
        return res
    finally:
        CS.kmeans_many = saved


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identify_bench.txt"))
    ap.add_argument("--model_type", default="vit_b")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    import torch
    import transformers
    from gaussmart_amd import camera_select as CS
    from gaussmart_amd import identify_cli, sam as S, segment_cli
    dev = torch.device(args.device)
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def sync():
        torch.cuda.synchronize(dev)

    try:
        import sklearn
        have_sklearn = sklearn.__version__
    except ImportError:
        have_sklearn = None
    say(f"view selection and gaussmart_amd.identify_cli on {torch.cuda.get_device_name(dev)}; torch {torch.__version__}, transformers "
        f"{transformers.__version__}, numpy {np.__version__}, scikit-learn {have_sklearn or 'not importable'}; "
        f"{os.environ.get('OMP_NUM_THREADS', 'unset')} OMP threads")
    say(f"median of {args.repeats} timed calls after {args.warmup} warm-up calls, (min .. max), wall clock with the device synchronised")
    say(" step 1, select_representative_cameras (k = 3 .. 15, 10 initialisations each):")
    for n in (49, 300, 1000):
        views = dome_views(n, n)
        d_ms, d_lo, d_hi, got = timed(lambda: CS.select_representative_cameras(views, device=dev), args.warmup, args.repeats, sync)
        h_ms, h_lo, h_hi, want = timed(lambda: CS.select_representative_cameras(views), args.warmup, args.repeats)
        say(f"  N = {n:4d}  device (one launch of 130 fits)   {d_ms:9.3f} ms  ({d_lo:.3f} .. {d_hi:.3f})")
        say(f"            numpy twin                        {h_ms:9.3f} ms  ({h_lo:.3f} .. {h_hi:.3f})   same selection: {got == want}")
        if have_sklearn:
            s_ms, s_lo, s_hi, ref = timed(lambda: sklearn_select(views), 1, max(3, args.repeats // 2))
            say(f"            scikit-learn KMeans (140 fits)    {s_ms:9.3f} ms  ({s_lo:.3f} .. {s_hi:.3f})   same selection: "
                f"{ref['selected_indices'] == want['selected_indices']}")
        # the parts of the device route
        pos, _ = CS.camera_centres_dirs(views)
        X = CS.normalize_positions(pos)[0]
        Xc = X - X.mean(axis=0)
        ks = list(range(3, 16))

        def draw():
            c0 = np.zeros((130, 16, 3))
            for j, k in enumerate(ks):
                rs = np.random.RandomState(42)
                for i in range(10):
                    c0[10 * j + i, :k] = CS.kmeans_pp_init(Xc, k, rs)
            return c0
        i_ms, _, _, c0 = timed(draw, 1, args.repeats)
        fit_k = np.repeat(np.asarray(ks, np.int32), 10)
        tol = float(np.mean(np.var(X, axis=0)) * CS.TOL)
        l_ms, l_lo, l_hi, res = timed(lambda: CS.lloyd_batch(Xc, c0, fit_k, tol, device=dev), args.warmup, args.repeats, sync)
        t_ms, _, _, twin = timed(lambda: CS.lloyd_batch_host(Xc, c0, fit_k, tol), 1, max(3, args.repeats // 2))
        equal = all(np.array_equal(res[key], twin[key]) for key in res)
        say(f"            parts: k-means++ draws on the host {i_ms:.3f} ms; lloyd_batch (upload, launch, read-back) {l_ms:.3f} ms "
            f"({l_lo:.3f} .. {l_hi:.3f}); lloyd_batch_host {t_ms:.3f} ms; bit-equal: {equal}; iterations {int(res['n_iter'].min())} .. "
            f"{int(res['n_iter'].max())}")

    # the whole command
    say(f" the command on a synthetic dtu scan: 49 cameras, 1024x768 pictures, 100000 points, SAM {args.model_type} with random weights, "
        "32 x 32 points, decoder hip, --clean:")
    from PIL import Image
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        scan, out = os.path.join(tmp, "scan"), os.path.join(tmp, "out")
        os.makedirs(os.path.join(scan, "images"))
        views = dome_views(49, 49)
        yy, xx = np.mgrid[0:768, 0:1024]
        mats = {}
        for i, v in views.items():
            img = np.stack([(xx + 13 * i) % 256, (yy * 2 + 7 * i) % 256, ((xx // 64 + yy // 64 + i) % 2) * 200], -1).astype(np.uint8)
            img[200:500, 300 + 5 * i:700] = (250, 30, 30)
            Image.fromarray(img).save(os.path.join(scan, "images", f"{i:04d}.jpg"), quality=90)
            for key in ("world_mat", "scale_mat", "camera_mat"):
                mats[f"{key}_{i}"] = v[key]
        np.savez(os.path.join(scan, "cameras.npz"), **mats)
        segment_cli.write_cloud_ply(os.path.join(scan, "points.ply"), rng.normal(size=(100000, 3)) * 0.3, np.full((100000, 3), 128, np.uint8))
        weights = S.random_sam_weights(S.SamConfig.preset(args.model_type), seed=0)
        gen = S.SamMaskGenerator(weights, points_per_side=32, pred_iou_thresh=-100.0, stability_score_thresh=0.0, device=dev, decoder="hip")
        cli = identify_cli.parser().parse_args(["-s", scan, "-o", out, "-t", "dtu", "--clean", "--overwrite", "--device", str(dev)])
        for run in range(2):          # the second run has every kernel loaded
            text = []
            t0 = time.perf_counter()
            identify_cli.run(cli, generator=gen, echo=text.append)
            sync()
            total = 1e3 * (time.perf_counter() - t0)
        steps = [json.loads(t) for t in text]
        for s in steps[:5]:
            extra = ""
            if s["step"] == 1:
                extra = f"   ({s['cameras']} cameras -> {s['selected']} views, best k {s['best_k']})"
            if s["step"] == 2:
                per = s["views"]
                extra = (f"   ({len(per)} views; per view: embed {statistics.median(v['embed_ms'] for v in per):.1f}, decode "
                         f"{statistics.median(v['decode_ms'] for v in per):.1f}, select {statistics.median(v['select_ms'] for v in per):.1f} ms; "
                         f"{statistics.median(v['masks'] for v in per):.0f} masks; the rest is reading the picture and writing the .npz)")
            if s["step"] == 3:
                extra = f"   ({s['points_in']} -> {s['points']} points)"
            if s["step"] == 4:
                extra = f"   ({s['labelled']} labelled, {s['segments']} segments)"
            say(f"  step {s['step']} {s['name']:<14s} {s['ms']:10.3f} ms{extra}")
        say(f"  whole command (second run)  {total:10.3f} ms")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
