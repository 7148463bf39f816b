"""render_bwd's compacting scan front: a wave scans the touch words of its tile list in chunks of 64 positions, keeps the
positions whose nibble for its own 8x8 quad is set in a 128-entry ring, and replays batches of 64 TOUCHED entries
(gaussmart_amd/csrc/render_bwd.hip).  The scenes below put that front where it can go wrong:

  * small faint splats in long lists: a quad's touched entries are sparse, one batch spans many scan chunks, and a chunk
    that holds more touched entries than the batch still needs is consumed in two fills;
  * large splats: nearly every entry is touched, a chunk is a batch and compaction is the identity;
  * few tiles with lists of several thousand entries: the ring (128 entries) wraps dozens of times;
  * frames whose width and height are not multiples of 16 (quads partly or wholly outside the frame).

Gradients of all seven allmap channels and the colour are held to the fp64 oracle with the bars of
tests/test_gpu_rasterizer.py (oracle_farm.check_gradient_bars: relative to the oracle's own formulas evaluated in fp32 on the
same scene).  Those bars cap a row at FLIP_CAP = 2 x FLIP_LEVEL_MAX, the largest error the fp32 ORACLE shows on any row of the
cases the cap was derived from (tests/golden/oracle_flip_levels.json); a scene on which the fp32 oracle itself is off by more
than that level on some row -- one sub-pixel, faint, nearly edge-on splat is enough: seed 25 of the 41x27 scene and seed 21 of
the 96x80 one have such a row at 1.1e-2 and 1.7e-2 of the scale in `scales` -- lies outside what the cap can judge.  The seeds
below were picked on the CPU by that criterion alone (fp32 oracle vs fp64 oracle, worst row of any tensor: 6e-5 .. 6.5e-4), and
the parity test asserts it as a precondition before it looks at the kernel's figures.  The 16-float-record kernel (no surface gradient) must equal the general one bit for bit on the same scenes,
and the same backward run twice must give identical bits.  Call sites protected: train.py:144 (total_loss.backward())."""
import pytest
import torch

from conftest import hip_settings, facing_scene
from gaussmart_amd.synthetic import activate
from oracle_farm import spec, run_case, compare_case, check_gradient_bars, FLIP_LEVEL_MAX
from test_gpu_rasterizer import _hip_gradients, _to

pytestmark = pytest.mark.gpu

ST = (1e-3,)      # the margin at which the oracle names the flip-sensitive Gaussians of a case
# name -> (n, w, h, seed, radius_px, opacity shift (logit), constant opacity)
SCENES = {
    "sparse-small-splats-30k@96x80-r2": (30000, 96, 80, 31, 2.0, 0.0, 0.03),
    "dense-large-splats-3k@96x80-r24": (3000, 96, 80, 22, 24.0, 0.0, 0.05),
    "ring-wraps-24k@48x48-r5": (24000, 48, 48, 23, 5.0, -3.0, None),
    "odd-frame-8k@75x53-r7": (8000, 75, 53, 24, 7.0, -2.0, None),
    "odd-frame-sparse-12k@41x27-r2.5": (12000, 41, 27, 26, 2.5, 0.0, 0.04),
}
# (not registered with the session's oracle farm: its committed checksum and flip-level files list the farm's cases, and
# FLIP_CAP is derived from them.  The oracle side of these five cases runs in this process, 10-25 s each.)
SPECS = {"compaction-" + name: spec("facing", n, w, h, seed, radius_px=r, flags=3, opa_shift=shift, opa_const=const,
                                    wseed=seed + 11, sens_tols=ST)
         for name, (n, w, h, seed, r, shift, const) in SCENES.items()}


def _oracle(sp, monkeypatch):
    threads = torch.get_num_threads()
    monkeypatch.setenv("FARM_TORCH_THREADS", str(max(1, min(8, threads))))
    try:
        res = run_case(sp)
    finally:
        torch.set_num_threads(threads)
    res["grads"] = {k: torch.from_numpy(v) for k, v in res["grads"].items()}
    res["d32"] = {k: torch.from_numpy(v) for k, v in res["d32"].items()}
    return res


@pytest.mark.parametrize("case", sorted(SPECS))
def test_backward_parity_compacted_batches(gpu_device, monkeypatch, case):
    """Every input's gradient against the fp64 oracle (all seven allmap channels carry gradient: the general kernel)."""
    sp = SPECS[case]
    gh, c_h, radii_h, _ = _hip_gradients(sp, gpu_device)
    res = _oracle(sp, monkeypatch)
    # precondition on the SCENE (module docstring): the fp32 oracle stays inside the level FLIP_CAP was derived from, on every row
    level32 = max(float(res["d32"][k].max()) / float(res["grads"][k].abs().max()) for k in res["d32"])
    assert level32 <= FLIP_LEVEL_MAX, (case, level32)
    stats, stats32, flips = compare_case(res, gh, radii_h)
    c_o = torch.from_numpy(res["color"])
    mean, longest, walked = (res["lists"][k] for k in ("mean", "max", "walked"))
    print(f"\n[{case}] tile lists: mean {mean:.0f}, max {longest} entries; deepest entry any pixel blends: {walked}; "
          f"fp32 oracle's worst row: {level32:.2e} of the scale")
    # the front has work to do: lists several rings long, walked to several batches' depth
    assert longest >= 4 * 128 or "dense" in case
    assert walked >= 256
    assert float((c_h - c_o).abs().max()) < 5e-3
    check_gradient_bars(case, stats, stats32, flips=flips)


def _scene(name, dev):
    n, w, h, seed, r, shift, const = SCENES[name]
    p, cam = facing_scene(n, w, h, seed=seed, radius_px=r)
    p = dict(p)
    p["opacity"] = p["opacity"] + shift
    a = activate(p)
    if const is not None:
        a["opacities"] = torch.full_like(a["opacities"], const)
    g = torch.Generator().manual_seed(seed + 5)
    wc, wa = torch.randn(3, h, w, generator=g).to(dev), torch.randn(7, h, w, generator=g).to(dev)
    return _to(a, dev), cam, n, wc, wa


def _backward(a, cam, n, dev, loss):
    from gaussmart_amd.rasterizer import GaussianRasterizer
    ins = {k: v.clone().requires_grad_(True) for k, v in a.items()}
    m2d = torch.zeros(n, 3, device=dev, requires_grad=True)
    c, r, am = GaussianRasterizer(hip_settings(cam, 3, (0.1, 0.2, 0.3), dev))(
        means3D=ins["means3D"], means2D=m2d, shs=ins["shs"], opacities=ins["opacities"], scales=ins["scales"],
        rotations=ins["rotations"])
    loss(c, am).backward()
    torch.cuda.synchronize()
    return [c.detach(), am.detach(), r] + [ins[k].grad for k in ins] + [m2d.grad]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_same_backward_twice_gives_identical_bits(gpu_device, name):
    """The ring, the partial chunks and the batch boundaries are a function of the touch words alone: two runs agree bit
    for bit, for the general kernel and for the 16-float-record one."""
    a, cam, n, wc, wa = _scene(name, gpu_device)
    for loss in (lambda c, am: (c * wc).sum() + (am * wa).sum(), lambda c, am: (c * wc).sum()):
        x, y = _backward(a, cam, n, gpu_device, loss), _backward(a, cam, n, gpu_device, loss)
        assert all(float(g.abs().max()) > 0 for g in x[3:])
        for u, v in zip(x, y):
            assert torch.equal(u, v)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_surface_kernel_equals_the_general_one_on_compacted_batches(gpu_device, monkeypatch, name):
    """The kernel for backwards without surface gradient keeps the entry's list position beside its 16-float record;
    its gradients must equal the general kernel's (position in the record), fed a zero dL/dallmap, bit for bit."""
    from gaussmart_amd import rasterizer as R
    a, cam, n, wc, _ = _scene(name, gpu_device)
    outs = []
    for fast in (True, False):
        monkeypatch.setattr(R, "_NO_SURFACE_FAST_PATH", fast)
        outs.append(_backward(a, cam, n, gpu_device, lambda c, am: (c * wc).sum()))
    assert all(float(g.abs().max()) > 0 for g in outs[0][3:])
    for u, v in zip(*outs):
        assert torch.equal(u, v)
