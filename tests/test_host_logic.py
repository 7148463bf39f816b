"""Host-side logic that needs no GPU: the per-model hand-over slots of the operator, the row-scan job's life cycle, the
oracle farm (a case end to end in this process, the committed checksums, the bar arithmetic), the trainer's decision which
allmap channels an iteration needs, and the schedule script's presets."""
import math
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_raster_state_slots_are_per_object():
    from gaussmart_amd.rasterizer import RasterState
    a, b = RasterState(), RasterState()
    a.set_pending_param_event("event-a", "stream-a")
    a.color_grad = "record-a"
    assert b.pending is None and b.color_grad is None            # nothing is shared between two models' states
    assert a.pop_pending() == ("event-a", "stream-a") and a.pop_pending() is None
    assert a.take_color_grad() == "record-a" and a.take_color_grad() is None
    from gaussmart_amd.gaussian_model import GaussianModel
    m1, m2 = GaussianModel(3, device="cpu"), GaussianModel(3, device="cpu")
    assert isinstance(m1.raster_state, RasterState) and m1.raster_state is not m2.raster_state
    import gaussmart_amd.rasterizer as R
    for name in ("_PENDING_PARAM_EVENT", "_ROW_SCAN_JOB", "_COLOR_GRAD"):      # round 3's module-level dicts are gone
        assert not hasattr(R, name)


def test_row_scan_job_is_found_through_the_image_and_retired(monkeypatch):
    """take_row_scan_job hands a job out once, only for the image of ITS forward, only on the stream it was ordered on, and
    never after the rasterizer's backward retired it."""
    import gaussmart_amd.rasterizer as R
    stream = types.SimpleNamespace(cuda_stream=1234)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: stream)

    def image_with(job):
        return types.SimpleNamespace(grad_fn=types.SimpleNamespace(row_scan_job=job), device="cuda:0")

    job = types.SimpleNamespace(_taken=False, _dead=False, _stream=1234)
    assert R.take_row_scan_job(image_with(job)) is job and job._taken
    assert R.take_row_scan_job(image_with(job)) is None                          # handed out once
    assert R.take_row_scan_job(types.SimpleNamespace(grad_fn=None, device="cuda:0")) is None      # a derived / foreign tensor
    other = types.SimpleNamespace(_taken=False, _dead=False, _stream=99)
    assert R.take_row_scan_job(image_with(other)) is None and not other._taken   # ordered on another stream
    dead = types.SimpleNamespace(_taken=False, _dead=True, _stream=1234)
    assert R.take_row_scan_job(image_with(dead)) is None
    assert R.row_scan_job_alive(job) and not R.row_scan_job_alive(dead) and not R.row_scan_job_alive(None)
    # the objective's check before its second half: alive and on the stream the job was ordered on
    assert R.row_scan_job_usable(job, 1234) and not R.row_scan_job_usable(job, 99)
    assert not R.row_scan_job_usable(dead, 1234) and not R.row_scan_job_usable(None, 1234)
    # the rasterizer's backward retires the job whether it can use it or not, and lets its lease go
    real = R._RowScanJob("lease", 1234)
    assert R.take_row_scan_job(image_with(real)) is real and real.stage == 0
    assert not R._retire_row_scan_job(real, 99) and real._dead and real._lease is None
    assert not R.row_scan_job_usable(real, 1234) and R.take_row_scan_job(image_with(real)) is None
    assert R._retire_row_scan_job(job, 1234) and not R.row_scan_job_alive(job)


def test_factored_gradient_needs_a_state_and_cpu_tensors_are_refused():
    import gaussmart_amd.rasterizer as R
    with pytest.raises(ValueError):
        R.rasterize_gaussians_raw(torch.zeros(1, 3), None, None, None, None, None, None, None, factored_sh_grad=True)


def test_oracle_farm_case_in_process_and_bar_arithmetic():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_farm as F
    sp = F.spec("facing", 120, 48, 32, 3, sens_tols=(1e-3,))
    a, cam, bg, wc, wa = F.build_inputs(sp)
    b = F.build_inputs(sp)[0]
    assert all(torch.equal(a[k], b[k]) for k in a)                # seeded: the HIP side and a worker see the same bits
    res = F.run_case(sp)
    assert set(res["grads"]) == {"means3D", "opacities", "shs", "scales", "rotations", "means2D"}
    assert res["grads"]["shs"].shape == (120, 16, 3) and res["color"].shape == (3, 32, 48)
    assert set(res["d32"]) == set(res["grads"]) and 1e-3 in res["sens"] and res["sens"][1e-3][0].shape == (120,)
    go = {k: torch.from_numpy(v) for k, v in res["grads"].items()}
    # the fp32 oracle is within its own bars, a corrupted gradient is not
    n = 120
    stable = torch.ones(n, dtype=torch.bool)
    s32 = {k: F.summarize(None, go[k], n, rows=stable, d=torch.from_numpy(res["d32"][k]), trim=F.TRIM(n)) for k in go}
    same = {k: F.summarize(go[k], go[k], n, rows=stable, trim=F.TRIM(n)) for k in go}
    assert F.check_gradient_bars("unit", same, s32) == 0.0
    bad = {k: F.summarize(go[k] * 1.01, go[k], n, rows=stable, trim=F.TRIM(n)) for k in go}
    with pytest.raises(AssertionError):
        F.check_gradient_bars("unit-bad", bad, s32)
    del F.REPORT[:]
    # trimmed maximum: one wild row is left out of the norm-wise figure and reported on its own
    g = torch.ones(1000, 3)
    h = g.clone(); h[7] += 0.5
    st = F.summarize(h, g, 1000, trim=1)
    assert st["normwise"] == 0.0 and math.isclose(st["trimmed_max"], 0.5, rel_tol=1e-6)


def test_gradient_bars_notice_a_subtly_wrong_kernel(monkeypatch):
    """What the gradient bars would let through, measured with the oracle evaluated in fp32 standing in for the HIP side,
    through the same compare_case + check_gradient_bars the GPU parity tests use.  (a) Unchanged, it passes.  (b) With every
    flip-sensitive row of every tensor scaled by 1.001 -- a relative error of 1e-3, ten times north_star's figure, on a fifth
    of all Gaussians -- it is rejected (the bars before the flip-row median / p90 let it pass with a worst usage of 0.32).
    (c) With one threshold constant of the walk wrong on the fp32 side only, it is rejected by at least one of the two cases."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_farm as F
    import test_gpu_rasterizer as TR
    from oracle import surfel_ref as O
    cases = (TR.SH_SCALE_ROT[0], TR.CLAMP[3])
    assert cases == ("facing2k-s0-flags3", "clamp500-s3-flags3")
    wrong = dict(ALPHA_MAX=0.985, T_EPS=1.2e-4, ALPHA_MIN=1 / 255.5, FILTER_INV_SQUARE=2.02, NEAR_N=0.25)
    true = {name: getattr(O, name) for name in wrong}
    threads = torch.get_num_threads()
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 2
    monkeypatch.setenv("FARM_TORCH_THREADS", str(max(1, min(12, cores))))

    def rejected(case, gh, radii_h, res):
        stats, stats32, flips = F.compare_case(res, gh, radii_h)
        try:
            F.check_gradient_bars(case, stats, stats32, flips=flips)
        except AssertionError as e:
            return str(e)
        return None

    try:
        caught = {name: [] for name in wrong}
        for case in cases:
            sp = F.FARM.specs[case]
            res = F.run_case(sp, keep32=True)
            F.check_against_committed_checksums(case, res)
            g32 = {k: torch.from_numpy(v) for k, v in res["grads32"].items()}
            sens = F.flip_sensitive_rows(res, res["radii32"])
            assert 100 <= int(sens.sum()) <= sp["n"] // 2
            # (a) the fp32 oracle is inside every bar, with room
            stats, stats32, flips = F.compare_case(res, g32, res["radii32"])
            assert F.check_gradient_bars(case, stats, stats32, flips=flips) < 0.5
            # (b) a relative error of 1e-3 on the flip-sensitive rows alone
            scaled = {k: torch.where(sens.reshape([-1] + [1] * (v.dim() - 1)), v * 1.001, v) for k, v in g32.items()}
            why = rejected(case, scaled, res["radii32"], res)
            assert why is not None and "flip-sensitive rows: median" in why, (case, why)
            # (c) one wrong constant in the fp32 evaluation; the fp64 side (res) keeps the true ones
            a, cam, bg, wc, wa = F.build_inputs(sp)
            for name, value in wrong.items():
                setattr(O, name, value)
                try:
                    g_bad, _, _, r_bad, _ = F._oracle_once(sp, a, cam, bg, wc, wa, torch.float32)
                finally:
                    setattr(O, name, true[name])
                why = rejected(case, g_bad, r_bad, res)
                if why is not None:
                    caught[name].append(f"{case}: {why}")
        for name in wrong:
            assert caught[name], f"{name} = {wrong[name]} passes the gradient bars of both cases"
    finally:
        for name, value in true.items():
            setattr(O, name, value)
        torch.set_num_threads(threads)
        del F.REPORT[:]


def test_farm_refuses_more_workers_than_the_card_allows(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_farm as F
    farm = F.Farm()
    farm.register("tiny", F.spec("facing", 8, 16, 16, 0))
    monkeypatch.setenv("FARM_WORKERS", "5")
    with pytest.raises(AssertionError, match="processes-per-card"):
        farm.start()
    assert farm.pool is None and not farm.futures
    monkeypatch.setenv("FARM_WORKERS", "0")
    assert farm.start() == 0


def test_committed_oracle_checksums_cover_every_registered_case():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import json
    import oracle_farm as F
    import test_gpu_rasterizer, test_gpu_deep_lists, test_gpu_wide_payload      # noqa: F401  (register the cases)
    want = json.load(open(F.CHECKSUMS))
    assert set(F.FARM.specs) == set(want), sorted(set(F.FARM.specs) ^ set(want))
    for key, sums in want.items():
        for k, (s, sa) in sums.items():
            assert math.isfinite(s) and math.isfinite(sa) and sa >= 0.0, (key, k)   # (precomputed T + colours: dL/dmeans3D = 0)


def test_committed_flip_levels_cover_every_case_with_an_fp32_pass_and_set_the_cap():
    """tests/golden/oracle_flip_levels.json (written by tests/golden/make_oracle_flip_levels.py) holds the fp32 oracle's own
    error levels for every registered case with an fp32 pass, every tensor of it; FLIP_CAP is twice the file's largest
    flip-row figure and not above the 2e-2 it replaced."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import json
    import oracle_farm as F
    import test_gpu_rasterizer, test_gpu_deep_lists, test_gpu_wide_payload      # noqa: F401  (register the cases)
    levels = json.load(open(F.FLIP_LEVELS))
    want = {k for k, sp in F.FARM.specs.items() if sp["want32"]}
    assert set(levels) == want, sorted(set(levels) ^ want)
    checksums = json.load(open(F.CHECKSUMS))
    largest = 0.0
    for key, tensors in levels.items():
        assert set(tensors) == set(checksums[key]), key
        for k, t in tensors.items():
            assert t["flip_rows"] + t["stable_rows"] == F.FARM.specs[key]["n"], (key, k)
            for m in ("flip_max", "flip_median", "flip_p90", "stable_max", "stable_median", "stable_p90"):
                assert math.isfinite(t[m]) and t[m] >= 0.0, (key, k, m)
            largest = max(largest, t["flip_max"])
    assert F.flip_level_max()[0] == largest == F.FLIP_LEVEL_MAX
    assert F.FLIP_CAP == min(2e-2, 2.0 * largest) and F.FLIP_BIG < F.FLIP_CAP <= 2e-2


def test_trainer_asks_the_forward_for_the_channels_the_objective_reads(monkeypatch):
    """training_step's choice of color_only / no_dist_median follows train.py:132-133 (lambda_normal from iteration 7,000,
    lambda_dist from 3,000) and the reference's defaults (lambda_dist = 0, depth_ratio = 0)."""
    import gaussmart_amd.trainer as T
    from gaussmart_amd.params import OptimizationParams, PipelineParams
    seen = []

    class Stop(Exception):
        pass

    def fake_render(cam, g, pipe, bg, **kw):
        seen.append((kw.get("color_only"), kw.get("no_dist_median")))
        raise Stop

    monkeypatch.setattr(T, "render", fake_render)
    monkeypatch.setattr(T, "_use_factored_sh_grad", lambda *a: True)
    g = types.SimpleNamespace(update_learning_rate=lambda it: None, get_xyz=torch.zeros(1, 3), optimizer=None, active_sh_degree=3)
    for it, lam_n, lam_d, ratio in ((100, 0.05, 0.0, 0.0), (7001, 0.05, 0.0, 0.0), (7001, 0.0, 0.0, 0.0), (3001, 0.05, 100.0, 0.0),
                                    (2999, 0.05, 100.0, 0.0), (9000, 0.05, 0.0, 1.0)):
        opt, pipe = OptimizationParams(), PipelineParams()
        opt.lambda_normal, opt.lambda_dist, pipe.depth_ratio = lam_n, lam_d, ratio
        with pytest.raises(Stop):
            T.training_step(g, None, None, opt, pipe, None, it, render_fn=fake_render)
    assert seen == [(True, True), (False, True), (True, True), (False, False), (True, True), (False, False)]


def test_schedule_script_presets_match_bench():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench
    import full_schedule_train as FS
    for name in ("scan24", "bicycle", "headline"):
        p = bench.PRESETS[name]
        assert FS.PRESETS[name] == (p["gaussians"], p["width"], p["height"], p["radius_px"])


def test_bench_dump_outputs_budget_and_fixed_samples(tmp_path):
    """bench.py --dump-outputs: per-Gaussian arrays keep the same seeded rows, larger arrays a seeded sample of their
    elements, everything together fits the budget, and the same inputs give the same files."""
    import json
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    n = 200_000
    g = torch.Generator().manual_seed(3)
    per_g = {"xyz": torch.randn(n, 3, generator=g), "features_rest": torch.randn(n, 15, 3, generator=g),
             "radii": torch.randint(0, 9, (n,), generator=g, dtype=torch.int32)}
    other = {"render": torch.rand(3, 1080, 1920, generator=g), "allmap": torch.rand(7, 1080, 1920, generator=g),
             "loss_total": torch.tensor(0.25, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), per_g, other, n)
    names = sorted(list(per_g) + list(other))
    assert sorted(p.name for p in (tmp_path / "a").glob("*.npy")) == [f"{k}.npy" for k in names]
    loaded = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64_000_000
    assert all(loaded[k].dtype == np.float32 for k in names if k != "loss_total") and loaded["loss_total"].dtype == np.float64
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    assert man["render"]["shape"] == [3, 1080, 1920] and man["loss_total"]["sample"] is None
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:bench.DUMP_GAUSSIAN_ROWS].sort().values
    assert np.array_equal(loaded["xyz"], per_g["xyz"][rows].numpy())
    assert np.array_equal(loaded["radii"], per_g["radii"][rows].float().numpy())
    assert loaded["features_rest"].shape == (bench.DUMP_GAUSSIAN_ROWS, 15, 3)
    assert np.all(np.isin(loaded["allmap"], other["allmap"].numpy()))          # a sample of the elements, not a recomputation
    for k in names:
        assert np.array_equal(loaded[k], np.load(tmp_path / "b" / f"{k}.npy")), k


def test_loss_utils_refuses_what_it_does_not_implement():
    """gaussmart_amd.loss_utils (the reference's l1_loss / ssim signatures on the fused kernel): argument checks run before any
    device work, and a CPU tensor is refused -- there is no CPU path behind these names."""
    from gaussmart_amd import _lib, loss_utils as H
    a, b = torch.rand(3, 16, 16, requires_grad=True), torch.rand(3, 16, 16)
    with pytest.raises(ValueError):
        H.ssim(a, b, window_size=7)
    with pytest.raises(ValueError):
        H.ssim(a, b, size_average=False)
    with pytest.raises(ValueError):
        H.l1_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        H.l1_loss(a, b[:, :8])
    with pytest.raises(ValueError):
        H.ssim(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16))      # a batch: the kernel takes one image
    with pytest.raises(_lib.GsrError):
        H.l1_loss(a, b)
    with pytest.raises(_lib.GsrError):
        H.ssim(a[None], b[None])


def test_reference_objective_switch_keeps_the_torch_maps(monkeypatch):
    """PipelineParams.reference_objective: training_step asks render() for the torch-derived maps (surface_maps=True), i.e. the
    reference's own objective formulation, instead of the fused node on allmap."""
    import gaussmart_amd.trainer as T
    from gaussmart_amd.params import OptimizationParams, PipelineParams
    seen = []

    class Stop(Exception):
        pass

    def fake_render(cam, g, pipe, bg, **kw):
        seen.append(kw.get("surface_maps"))
        raise Stop

    g = types.SimpleNamespace(update_learning_rate=lambda it: None, get_xyz=types.SimpleNamespace(is_cuda=True), optimizer=None,
                              active_sh_degree=3)
    for flag in (False, True):
        opt, pipe = OptimizationParams(), PipelineParams()
        pipe.reference_objective = flag
        pipe.factored_sh_grad = False
        with pytest.raises(Stop):
            T.training_step(g, None, None, opt, pipe, None, 8000, render_fn=fake_render)
    assert seen == [False, True]
    # ... and it wins over the factored path (whose forward builds no maps for torch to read)
    pipe = PipelineParams()
    pipe.reference_objective = True
    g.raster_state, g.optimizer = object(), T.FusedAdam.__new__(T.FusedAdam)
    assert not T._use_factored_sh_grad(g, pipe, T.render, True)
    pipe.reference_objective = False
    assert T._use_factored_sh_grad(g, pipe, T.render, True)
