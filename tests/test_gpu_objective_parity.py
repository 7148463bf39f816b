"""loss.hip and regularizer.hip on the device, pixel by pixel, through the C ABI: gsr_loss_forward / _backward, gsr_regularizer_forward /
_backward / _backward_partials and gsr_objective_finish against the fp64 twins of tests/objective_cases.py, each quantity held to
the bar derived there (tests/test_objective_cpu.py proves every bar reachable and tight without a GPU).  Every output is pre-filled
with NaN: a slot or a pixel nobody writes shows.  GSR_OBJECTIVE_PARITY_REPORT=<file>: the measured errors and bars are appended
there (profiles/objective_parity.txt is such a run)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import objective_cases as OC
from objective_cases import E, U32, TINY32, bar, ratio
from gaussmart_amd import _lib
from gaussmart_amd._dev import ptr, stream

pytestmark = pytest.mark.gpu


def report(line):
    out = os.environ.get("GSR_OBJECTIVE_PARITY_REPORT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
    print(line)


@pytest.fixture
def held():
    """held(case, what, got, truth): max over the elements of |got - truth.v| / bar(truth) must be <= 1.  Every figure is printed
    before it is asserted; the case's worst quantity is reported -- one line per case -- whether the case holds or not."""
    rows = []

    def check(case, what, got, truth, where=None):
        got, want, b = got.detach().double().cpu(), truth.v, bar(truth)
        if where is not None:
            got, want, b = got[where], want[where], b[where]
        err = (got - want).abs()
        use = ratio(err, b)
        rows.append((use, what, float(err.max()) if err.numel() else 0.0, float(b.max()) if b.numel() else 0.0, case))
        print(f"{case} {what}: max err {rows[-1][2]:.3e}, max bar {rows[-1][3]:.3e}, worst err/bar {use:.3f}")
        assert bool(torch.isfinite(got).all()) and use <= 1.0, (case, what, use)

    yield check
    if rows:
        use, what, err, b, case = max(rows)
        report(f"{case}: {len(rows)} quantities, worst err/bar {use:.3f} at {what} (max err {err:.3e}, max bar {b:.3e})")


def nans(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


# ------------------------------------------------------------------------------------------------ photometric loss
@pytest.mark.parametrize("content,shape", OC.LOSS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_loss_forward_and_backward_per_pixel(gpu_device, held, content, shape):
    L, dev = _lib.lib(), gpu_device
    Cn, H, W = shape
    name = f"loss {content} {Cn}x{H}x{W}"
    xh, yh = OC.loss_inputs(content, shape)
    x, y = xh.to(dev), yh.to(dev)
    fwd, bwd = OC.loss_truth(content, shape)
    n_slots = OC.num_slots(H, W)
    assert L.gsr_loss_num_partials(H, W) == 2 * n_slots
    maps, partials = nans((3, Cn, H, W), dev), nans((n_slots, 2), dev)
    _lib.check(L.gsr_loss_forward(ptr(x), ptr(y), Cn, H, W, ptr(maps), ptr(partials), stream(dev)))
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(maps).all()) and bool(torch.isfinite(partials).all())        # every pixel and every slot was written
    for k, what in enumerate(("dS/dmu1", "dS/dE[x2]", "dS/dE[xy]")):
        held(name, what, maps[k], fwd["maps"][k])
    g16y, g16x = -(-H // 16), -(-W // 16)
    slots = partials.reshape(g16y, g16x, 2).cpu()
    top_left = torch.zeros(g16y, g16x, dtype=torch.bool)
    top_left[::2, ::2] = True
    for k, what in enumerate(("sum S", "sum |x-y|")):
        held(name, f"{what} per tile", slots[..., k], fwd["slots"][k], where=top_left)
        assert bool((slots[..., k][~top_left] == 0.0).all()), what           # a tile's other cells hold exactly 0
        total = E(fwd["slots"][k].v.sum(), fwd["slots"][k].b.sum())
        held(name, f"{what} total", slots[..., k].double().sum(), total)

    same = (xh == yh)
    runs = {}
    for (lam, gs), truth in bwd.items():
        scale = torch.tensor([gs], dtype=torch.float32, device=dev)
        out = []
        for _ in range(2):
            dimg = nans((Cn, H, W), dev)
            _lib.check(L.gsr_loss_backward(ptr(x), ptr(y), ptr(maps), Cn, H, W, lam, ptr(scale), ptr(dimg), stream(dev)))
            out.append(dimg)
        torch.cuda.synchronize(dev)
        held(name, f"dimg lambda {lam} scale {gs}", out[0], truth)
        assert torch.equal(out[0], out[1])                                   # the same call twice: the same bits
        runs[(lam, gs)] = out[0].cpu()
    # sign(0) = 0: where x == y the L1 part is exactly absent.  With lambda = 0 nothing is left; otherwise what is left is the
    # lambda = 1 run's value times lambda: k_ssim = (-lambda / n) gs against (-1 / n) gs and one product each, five roundings
    if bool(same.any()):
        for gs in OC.LOSS_GRAD_SCALES:
            assert float(runs[(0.0, gs)][same].abs().max()) == 0.0
            ref = OC.f32(0.2) * runs[(1.0, gs)][same].double()
            assert bool(((runs[(0.2, gs)][same].double() - ref).abs() <= 6 * U32 * ref.abs() + TINY32).all())


# ------------------------------------------------------------------------------------------------ surface regularizers
@pytest.mark.parametrize("case", OC.REG_CASES, ids=OC.reg_case_id)
def test_regularizer_forward_and_backward_per_pixel(gpu_device, held, case):
    L, dev = _lib.lib(), gpu_device
    kind, size, r, (ln, ld) = case
    H, W = size
    name = "reg " + OC.reg_case_id(case)
    amh = OC.reg_allmap(kind, size)
    am = amh.to(dev)
    kinv = (C.c_float * 9)(*OC.reg_kinv(size).reshape(-1).tolist())
    truth = OC.reg_truth(case)
    n_slots = OC.num_slots(H, W)
    gs = OC.REG_GRAD_SCALE
    scale = torch.tensor([gs], dtype=torch.float32, device=dev)
    p_fwd, p_bwd = nans((n_slots, 2), dev), nans((n_slots, 2), dev)
    dam, dam_p = nans((7, H, W), dev), nans((7, H, W), dev)
    _lib.check(L.gsr_regularizer_forward(ptr(am), H, W, kinv, r, ptr(p_fwd), stream(dev)))
    _lib.check(L.gsr_regularizer_backward(ptr(am), H, W, kinv, r, ln, ld, ptr(scale), ptr(dam), stream(dev)))
    _lib.check(L.gsr_regularizer_backward_partials(ptr(am), H, W, kinv, r, ln, ld, ptr(scale), ptr(dam_p), ptr(p_bwd), stream(dev)))
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(p_fwd).all()) and bool(torch.isfinite(dam).all())             # every slot, every pixel, holes included
    assert torch.equal(p_fwd, p_bwd) and torch.equal(dam, dam_p)
    slots = p_fwd.reshape(-(-H // 16), -(-W // 16), 2).cpu()
    held(name, "sum error per tile", slots[..., 0], truth["sums"][0])
    held(name, "sum distortion per tile", slots[..., 1], truth["sums"][1])
    lit = amh[1] > 0
    got = dam.cpu()
    for c in range(7):
        held(name, f"d_allmap[{c}] lit", got[c], truth["dam"][c], where=lit)
        held(name, f"d_allmap[{c}] holes", got[c], truth["dam"][c], where=~lit)
    # the contract at pixels without a splat: (finite, above) zero in channels 0 and 1, channel 6 = kd -- at every pixel, to the bit
    assert float(got[0][~lit].abs().sum()) == 0.0 and float(got[1][~lit].abs().sum()) == 0.0
    kd = np.float32(np.float32(ld) * (np.float32(1.0) / (np.float32(W) * np.float32(H)))) * np.float32(gs)
    assert bool((got[6] == float(kd)).all())
    if kind == "island":
        # the lit pixel's cross product is exactly 0 (all four neighbours are holes): reg_bwd_kernel hands nothing to them
        assert float(got[[0, 1, 5]].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ objective finish
@pytest.mark.parametrize("with_reg", [False, True], ids=["loss", "loss+reg"])
@pytest.mark.parametrize("n", OC.FINISH_N)
def test_objective_finish_on_synthetic_partials(gpu_device, held, n, with_reg):
    """It reads only counts from C, H, W: H = 16, W = 16 n gives n partial pairs; 2048 pairs make one round of the summation loop."""
    L, dev = _lib.lib(), gpu_device
    Cn, H, W = 3, 16, 16 * n
    lam, ln, ld = 0.2, 0.05, 100.0
    assert L.gsr_loss_num_partials(H, W) == 2 * n
    plh, prh = OC.finish_partials(n, with_reg)
    pl, pr = plh.to(dev), (prh.to(dev) if with_reg else None)
    out = nans((5,), dev)
    _lib.check(L.gsr_objective_finish(ptr(pl), Cn, H, W, ptr(pr), lam, ln, ld, ptr(out), stream(dev)))
    torch.cuda.synchronize(dev)
    truth = OC.finish_truth(plh, prh, Cn, H, W, lam, ln, ld)
    for k, what in enumerate(("total", "l1", "ssim", "normal", "dist")):
        held(f"finish n {n} {'with' if with_reg else 'without'} reg", what, out[k], truth[k])
    if n == 2049:
        # the same five scalars from the workgroup that rides along with loss_bwd_kernel
        img, maps, dimg, out2 = torch.zeros(Cn, H, W, device=dev), torch.zeros(3, Cn, H, W, device=dev), nans((Cn, H, W), dev), nans((5,), dev)
        scale = torch.ones(1, device=dev)
        _lib.check(L.gsr_loss_backward_finish(ptr(img), ptr(img), ptr(maps), Cn, H, W, lam, ptr(scale), ptr(dimg), ptr(pl), ptr(pr),
                                              ln, ld, ptr(out2), None, stream(dev)))
        torch.cuda.synchronize(dev)
        assert torch.equal(out, out2) and bool(torch.isfinite(dimg).all())
