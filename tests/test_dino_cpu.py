"""The host side of the DINO feature term (gaussmart_amd/dino.py, loss_utils.dino_loss, trainer.DinoTerm): the loader against
what transformers' save_pretrained writes, the RoPE table against the installed library's, dino_loss against values captured
from the reference's own function (tests/golden/dino_loss.npz, scripts/make_dino_loss_golden.py), and the trainer plumbing on
the host path with a stub encoder.  The kernels are tests/test_gpu_dino.py."""
import csv
import os
import types

import numpy as np
import pytest
import torch

import dino_cases as DC
from conftest import GOLDEN
from gaussmart_amd import dino as D
from gaussmart_amd.loss_utils import dino_loss


def test_config_defaults_are_vit_b16():
    c = D.DinoConfig()
    assert (c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.intermediate_size, c.num_register_tokens) == (768, 12, 12, 3072, 4)
    assert (c.rope_theta, c.layer_norm_eps) == (100.0, 1e-5)
    assert (c.query_bias, c.key_bias, c.value_bias, c.proj_bias, c.mlp_bias, c.use_gated_mlp, c.hidden_act) == \
        (True, False, True, True, True, False, "gelu")
    assert c.image_mean == (0.485, 0.456, 0.406) and c.image_std == (0.229, 0.224, 0.225)
    assert c.tokens(1200, 1600) == 7505
    with pytest.raises(NotImplementedError):
        D.DinoConfig(hidden_size=96, num_attention_heads=2).check()
    with pytest.raises(NotImplementedError):
        D.DinoConfig(use_gated_mlp=True).check()


def test_loader_round_trip_with_the_librarys_own_files(tmp_path):
    from transformers import DINOv3ViTModel
    cfg = DC.config("A")
    torch.manual_seed(3)
    model = DINOv3ViTModel(cfg.to_hf()).eval()
    with torch.no_grad():
        for p in model.parameters():          # fp16-representable values, so that the loader's .half() is exact
            p.copy_((p + 0.05 * torch.randn_like(p)).half().float())
    model.save_pretrained(tmp_path)
    with open(tmp_path / "preprocessor_config.json", "w") as f:
        f.write('{"image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225]}')
    w = D.load_dino_weights(tmp_path)
    assert w.config.hidden_size == 128 and w.config.num_hidden_layers == 2 and w.config.key_bias is False
    sd = model.state_dict()
    assert set(w.tensors) == set(sd) - {"embeddings.mask_token"}
    for k, t in w.tensors.items():
        assert t.dtype == torch.float16 and torch.equal(t.float(), sd[k]), k
    x = DC.images(48, 80)
    mean, std = torch.tensor(cfg.image_mean).view(1, 3, 1, 1), torch.tensor(cfg.image_std).view(1, 3, 1, 1)
    with torch.no_grad():
        want = model((x - mean) / std)
    last, pooled = D.dino_host(w, x, torch.float32)
    assert torch.equal(last, want.last_hidden_state) and torch.equal(pooled, want.pooler_output)
    # our own writer is read back the same
    D.save_dino_weights(w, tmp_path / "again")
    w2 = D.load_dino_weights(tmp_path / "again")
    assert all(torch.equal(w2.tensors[k], t) for k, t in w.tensors.items())


def test_loader_refuses_hub_names_and_missing_files(tmp_path, monkeypatch):
    import socket

    def no_network(*a, **k):
        raise AssertionError("the loader touched the network")
    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        D.load_dino_weights("facebook/dinov3-vitb16-pretrain-lvd1689m")
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        D.DINOImageEncoder("facebook/dinov3-vitb16-pretrain-lvd1689m")
    with pytest.raises(FileNotFoundError, match="config.json"):
        D.load_dino_weights(tmp_path)
    D.save_dino_weights(DC.weights("A"), tmp_path)
    os.remove(tmp_path / "model.safetensors")
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        D.load_dino_weights(tmp_path)


@pytest.mark.parametrize("Hp,Wp", [(3, 5), (9, 14), (17, 16), (75, 100)])
def test_rope_table_and_patch_coordinates_match_the_library(Hp, Wp):
    from transformers.models.dinov3_vit import modeling_dinov3_vit as M
    coords = M.get_patches_center_coordinates(Hp, Wp, dtype=torch.float64, device=torch.device("cpu"))
    ours = D.patch_coordinates(Hp, Wp)
    assert ours.shape == coords.shape and float((ours - coords).abs().max()) <= 4 * 2.0 ** -53
    # the library's module computes in fp32; its formula in fp64:
    inv_freq = 1 / 100.0 ** torch.arange(0, 1, 4 / 64, dtype=torch.float64)
    angles = (2 * np.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2).tile(2)
    cos, sin = D.rope_table(Hp, Wp, 100.0)
    assert cos.shape == (Hp * Wp, 64)
    assert float((cos - torch.cos(angles)).abs().max()) <= 16 * 2.0 ** -53 and float((sin - torch.sin(angles)).abs().max()) <= 16 * 2.0 ** -53
    # ... and the module itself (fp32) agrees with the table to fp32 rounding of angles up to 2 pi
    rope = M.DINOv3ViTRopePositionEmbedding(DC.config("A").to_hf()).eval()
    c32, s32 = rope(torch.zeros(1, 3, 16 * Hp, 16 * Wp))
    assert float((c32.double() - cos).abs().max()) < 1e-5 and float((s32.double() - sin).abs().max()) < 1e-5


class _Stub:
    """encode_tensor hands back the queued embeddings, as the capture script's stub does."""

    def __init__(self, *embs):
        self.queue = list(embs)

    def encode_tensor(self, image):
        return self.queue.pop(0)


def test_dino_loss_matches_the_reference_values():
    z = np.load(os.path.join(GOLDEN, "dino_loss.npz"))
    n, negative = int(z["n_cases"]), 0
    assert n >= 6
    img = torch.zeros(3, 16, 16)
    for i in range(n):
        a, b, lam, golden = torch.from_numpy(z[f"a{i}"]), torch.from_numpy(z[f"b{i}"]), float(z[f"lambda{i}"]), float(z[f"golden{i}"])
        ours = dino_loss(img, img, _Stub(a, b), lam)
        assert ours.dtype == torch.float16 and ours.dim() == 0 and not ours.requires_grad
        a64, b64 = a.double(), b.double()
        cos64 = float((a64 @ b64) / (a64.norm().clamp_min(1e-8) * b64.norm().clamp_min(1e-8)))
        v64 = float(torch.tensor(lam, dtype=torch.float16)) * cos64
        assert abs(float(ours) - golden) <= abs(golden - v64) + 2.0 ** -11 * abs(v64), (i, float(ours), golden, v64)
        if cos64 < 0 and lam == 0.05:
            negative += 1
            assert float(ours) != 0.05 * cos64 and float(torch.tensor(0.05, dtype=torch.float16)) != 0.05
    assert negative >= 1


# ---------------------------------------------------------------- trainer plumbing on the host path
class _MeanEncoder:
    """A stand-in with the reference's interface: the embedding is a fixed random projection of the 4x4-pooled image."""

    def __init__(self):
        self.proj = torch.randn(48, 32, generator=torch.Generator().manual_seed(9))
        self.calls = 0

    def encode_tensor(self, image):
        self.calls += 1
        return torch.nn.functional.adaptive_avg_pool2d(image.detach().float(), 4).reshape(-1) @ self.proj


def _host_training_run(monkeypatch, dino):
    import gaussmart_amd.trainer as T
    from gaussmart_amd.params import OptimizationParams, PipelineParams
    g = torch.Generator().manual_seed(0)
    H = W = 24
    param = torch.nn.Parameter(torch.randn(3, H, W, generator=g))
    normal = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    cams = [types.SimpleNamespace(original_image=torch.rand(3, H, W, generator=g), uid=i) for i in range(2)]

    def fake_render(cam, gm, pipe, bg, **kw):
        image = torch.sigmoid(param)
        return {"render": image, "rend_normal": normal * image.mean(), "surf_normal": normal, "rend_dist": image[:1] ** 2,
                "viewspace_points": param, "visibility_filter": None, "radii": None}

    opt_torch = torch.optim.Adam([param], lr=0.05)
    gm = types.SimpleNamespace(update_learning_rate=lambda it: None, get_xyz=torch.zeros(1, 3), optimizer=opt_torch,
                               active_sh_degree=3, oneupSHdegree=lambda: None)
    real_step = T.training_step
    monkeypatch.setattr(T, "training_step", lambda *a, **k: real_step(*a, render_fn=fake_render, **k))
    opt, pipe = OptimizationParams(), PipelineParams()
    opt.densify_until_iter = 0
    opt.lambda_dist = 10.0
    T.train(gm, cams, opt, pipe, torch.zeros(3), first_iter=7000, iterations=7003, final_iteration=30000, dino=dino)
    return param.detach().clone()


def test_trainer_logs_the_term_and_leaves_the_parameters_alone(monkeypatch, tmp_path):
    import gaussmart_amd.trainer as T
    enc = _MeanEncoder()
    path = tmp_path / "model" / "dino_loss_log.csv"
    term = T.DinoTerm(enc, lambda_dino=0.05, start_iter=7001, csv_path=str(path))
    with_term = _host_training_run(monkeypatch, term)
    monkeypatch.undo()
    without = _host_training_run(monkeypatch, None)
    assert torch.equal(with_term, without)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["iteration", "dino_loss", "total_loss", "l1_loss", "dist_loss", "normal_loss"]       # train.py:65
    assert [int(r[0]) for r in rows[1:]] == [7001, 7002, 7003]
    vals = np.array([[float(v) for v in r[1:]] for r in rows[1:]])
    assert vals[0, 0] == 0.0 and (vals[1:, 0] != 0.0).all()         # the term starts AFTER start_iter (train.py:119)
    assert (vals[:, 3] > 0).all() and (vals[:, 4] > 0).all()        # lambda_dist and lambda_normal are active past 7000
    # every logged term is an fp16 value, and the ground truth of a camera is encoded once
    assert all(float(np.float16(v)) == v for v in vals[:, 0])
    assert enc.calls <= 2 + 2
    # flush() emptied the call's rows; the buffer's own sixth column is the photometric part: total = sum of the parts
    term2 = T.DinoTerm(_MeanEncoder(), 0.05, 7001)
    monkeypatch.undo()
    _host_training_run(monkeypatch, term2)
    assert term2.rows() != []
    for it, d, total, l1, dist, normal, phot in term2.rows():
        assert abs(total - (phot + dist + normal + d)) <= 4 * 2.0 ** -24 * (abs(phot) + abs(dist) + abs(normal) + abs(d)), it
    assert [r[:6] for r in term2.rows()] == [tuple([int(r[0])] + [float(v) for v in r[1:]]) for r in rows[1:]]
