"""LPIPS without a GPU: the loader, the torch twin against the restatement of tests/lpips_cases.py (a golden vector of the
reference cannot exist: its LPIPS package needs torchvision and the network), and metrics_cli --host."""
import json
import os
import re

import numpy as np
import pytest
import torch

import lpips_cases as LC
from conftest import ROOT
from gaussmart_amd import losses
from gaussmart_amd import lpips as LP
from gaussmart_amd import metrics_cli

SIZES = {"vgg": [(16, 16), (35, 67), (64, 48)], "alex": [(31, 31), (35, 67), (64, 48)]}


@pytest.mark.parametrize("net_type", ["vgg", "alex"])
def test_loader_maps_keys_and_ignores_classifier(tmp_path, net_type, monkeypatch):
    import urllib.request
    def refuse(*a, **k):
        raise AssertionError("the loader reached for the network")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    monkeypatch.setattr(torch.hub, "download_url_to_file", refuse)
    monkeypatch.setattr(urllib.request, "urlopen", refuse)
    backbone, lin = LC.write_weight_files(tmp_path, net_type)
    ref = LC.weights(net_type)
    for got in (LP.load_lpips_weights(net_type, backbone, lin), LP.weights_from_dir(net_type, str(tmp_path))):
        assert got.net_type == net_type and len(got.conv_w) == len(LP.TRUNK[net_type]) and len(got.lin) == 5
        for a, b in zip(got.conv_w + got.conv_b + got.lin, ref.conv_w + ref.conv_b + ref.lin):
            assert a.dtype == torch.float32 and torch.equal(a, b)
        assert [v.numel() for v in got.lin] == list(LP.N_CHANNELS[net_type])


def test_loader_missing_file_names_both_files(tmp_path):
    backbone, lin = LC.write_weight_files(tmp_path, "vgg")
    with pytest.raises(FileNotFoundError, match=r"vgg16.*vgg\.pth"):
        LP.load_lpips_weights("vgg", backbone, str(tmp_path / "nowhere" / "vgg.pth"))
    with pytest.raises(FileNotFoundError, match="two local files"):
        LP.weights_from_dir("alex", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        LP.LPIPS("vgg")
    os.remove(backbone)
    torch.save({"features.0.weight": torch.zeros(64, 3, 3, 3)}, backbone)
    with pytest.raises(KeyError, match=r"features\.0\.bias"):
        LP.load_lpips_weights("vgg", backbone, lin)


def test_module_opens_no_url():
    for name in ("lpips.py", "metrics_cli.py"):
        text = open(os.path.join(ROOT, "gaussmart_amd", name)).read()
        code = re.sub(r'""".*?"""', "", text, flags=re.S)
        code = re.sub(r"#.*", "", code)
        for word in ("torch.hub", "urllib", "http", "requests", "load_state_dict_from_url", "import torchvision", "from torchvision"):
            assert word not in code, f"{name} mentions {word}"
    assert "hub" not in vars(LP) and "weights_only=True" in open(os.path.join(ROOT, "gaussmart_amd", "lpips.py")).read()


@pytest.mark.parametrize("net_type", ["vgg", "alex"])
def test_twin_equals_restatement_fp64(net_type):
    w = LC.weights(net_type)
    for H, W in SIZES[net_type]:
        x, y = (t.double()[None] for t in LC.image_pair(H, W))
        want, min_norm = LC.restated_lpips(x, y, w)
        got = LP.lpips_host(x, y, net_type=net_type, weights=w)
        assert got.shape == (1, 1, 1, 1) and got.dtype == torch.float64
        assert min_norm > 1.0, f"{net_type} {H}x{W}: a tapped feature norm of {min_norm} makes the division ill conditioned"
        assert float(want) > 0.0
        # both are fp64 evaluations of the same expression in different orders
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (net_type, H, W, float(got), float(want))
        assert LC.twin(net_type, H, W, torch.float64) == float(got)


@pytest.mark.parametrize("net_type", ["vgg", "alex"])
def test_fp32_twin_sits_near_fp64(net_type):
    for H, W in SIZES[net_type]:
        v64, v32 = LC.twin(net_type, H, W, torch.float64), LC.twin(net_type, H, W, torch.float32)
        print(f"{net_type} {H}x{W}: fp32 twin off by {abs(v32 - v64) / v64:.2e} relative")
        assert abs(v32 - v64) <= 7e-7 * v64


def test_value_range_is_passed_through():
    """[0,1] (metrics.py) and x2-1 (train.py:326) are different inputs to the same function: neither is rescaled."""
    w = LC.weights("alex")
    x, y = (t.double() for t in LC.image_pair(35, 67))
    a = float(LP.lpips_host(x, y, net_type="alex", weights=w))
    b = float(LP.lpips_host(x * 2 - 1, y * 2 - 1, net_type="alex", weights=w))
    want_b, _ = LC.restated_lpips((x * 2 - 1)[None], (y * 2 - 1)[None], w)
    assert abs(b - float(want_b)) <= 1e-12 * b and abs(a - b) > 1e-3 * a
    assert float(LP.lpips_host(x, x, net_type="alex", weights=w)) == 0.0
    assert LP.lpips_host(x[None], y[None], net_type="alex", weights=w).shape == (1, 1, 1, 1)


def test_refusals_on_the_host():
    w = LC.weights("alex")
    x, y = LC.image_pair(35, 67)
    with pytest.raises(NotImplementedError, match="squeeze"):
        LP.lpips_host(x, y, net_type="squeeze", weights=w)
    with pytest.raises(NotImplementedError, match="squeeze"):
        LP.LPIPS("squeeze", weights=w)
    with pytest.raises(ValueError, match="batch of 2"):
        LP.lpips_host(torch.stack([x, x]), torch.stack([y, y]), net_type="alex", weights=w)
    with pytest.raises(ValueError, match="below the alex"):
        LP.lpips_host(x[:, :30, :40], y[:, :30, :40], net_type="alex", weights=w)
    with pytest.raises(ValueError, match="weights of 'alex'"):
        LP.lpips_host(x, y, net_type="vgg", weights=w)
    with pytest.raises(_lib_error(), match="no CPU path"):
        LP.lpips(x, y, net_type="alex", weights=w)


def _lib_error():
    from gaussmart_amd import _lib
    return _lib.GsrError


def test_metrics_cli_host(tmp_path, capsys):
    model = str(tmp_path / "model")
    names = LC.write_model(model)
    assert metrics_cli.main(["-m", model, "--host"]) == 0
    assert "LPIPS is null" in capsys.readouterr().out
    full = json.load(open(os.path.join(model, "results.json")))
    per = json.load(open(os.path.join(model, "per_view.json")))
    assert list(full) == ["ours_30000"] and set(full["ours_30000"]) == {"SSIM", "PSNR", "LPIPS"}
    assert full["ours_30000"]["LPIPS"] is None
    assert set(per["ours_30000"]) == {"SSIM", "PSNR", "LPIPS"}
    for key in ("SSIM", "PSNR", "LPIPS"):
        assert list(per["ours_30000"][key]) == names             # sorted, whatever order the files were written in
    assert all(v is None for v in per["ours_30000"]["LPIPS"].values())
    ssims, psnrs = [], []
    for n in names:
        r, g = LC.load_pair(model, "ours_30000", n)
        ssims.append(float(losses.ssim(r, g)))
        psnrs.append(float(losses.psnr(r, g)))
        assert per["ours_30000"]["SSIM"][n] == pytest.approx(ssims[-1], rel=1e-6)
        assert per["ours_30000"]["PSNR"][n] == pytest.approx(psnrs[-1], rel=1e-6)
    assert full["ours_30000"]["SSIM"] == pytest.approx(float(torch.tensor(ssims).mean()), rel=1e-6)
    assert full["ours_30000"]["PSNR"] == pytest.approx(float(torch.tensor(psnrs).mean()), rel=1e-6)


def test_metrics_cli_host_lpips_and_failing_scene(tmp_path, capsys):
    model, broken = str(tmp_path / "model"), str(tmp_path / "broken")
    names = LC.write_model(model)
    os.makedirs(broken)
    wdir = tmp_path / "w"
    wdir.mkdir()
    LC.write_weight_files(wdir, "alex")
    assert metrics_cli.main(["-m", broken, model, "--host", "--lpips_dir", str(wdir), "--lpips_net", "alex"]) == 1
    err = capsys.readouterr().err
    assert "Unable to compute metrics for model" in err and "FileNotFoundError" in err
    assert not os.path.exists(os.path.join(broken, "results.json"))
    per = json.load(open(os.path.join(model, "per_view.json")))["ours_30000"]["LPIPS"]
    w = LC.weights("alex")
    vals = []
    for n in names:
        r, g = LC.load_pair(model, "ours_30000", n)
        vals.append(float(LP.lpips_host(r, g, net_type="alex", weights=w)))
        assert per[n] == pytest.approx(vals[-1], rel=1e-6)
    full = json.load(open(os.path.join(model, "results.json")))["ours_30000"]["LPIPS"]
    assert full == pytest.approx(float(torch.tensor(vals).mean()), rel=1e-6)
    assert metrics_cli.main(["-m", model, "--host", "--lpips_dir", str(tmp_path / "none")]) == 2
