"""gaussmart_amd.sam without a GPU: the two weight namings, the point grid, preprocess, the torch twins of the selection
against transformers' own helpers and a plain loop, the ABI version, and sam_host against SamVisionEncoder called directly."""
import os

import numpy as np
import pytest
import torch

import sam_cases as SC
from gaussmart_amd import _lib
from gaussmart_amd import sam as S


@pytest.fixture(scope="module")
def full_weights():
    return SC.weights("E1", 256)


def test_abi_version_is_18():
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    with open(os.path.join(root, "include", "gsr.h")) as f:
        text = f.read()
    assert "#define GSR_ABI_VERSION 18" in text and _lib.ABI_VERSION == 18
    assert (_lib.GSR_SAM_W_LAYER0, _lib.GSR_SAM_W_PER_LAYER, _lib.GSR_SAM_W_NECK) == (len(S.ENC_HEAD), len(S.ENC_LAYER), len(S.ENC_NECK))


def test_weights_round_trip_under_both_namings(full_weights, tmp_path):
    w = full_weights
    S.save_sam_weights(w, str(tmp_path / "hf"))
    a = S.load_sam_weights(str(tmp_path / "hf"))
    assert a.config == w.config and a.tensors.keys() == w.tensors.keys()
    assert all(torch.equal(a.tensors[k], w.tensors[k]) for k in w.tensors)
    # segment_anything's naming, built with the inverse map
    pth = {S.hf_to_pth(k): t.clone() for k, t in w.tensors.items() if S.hf_to_pth(k) is not None}
    assert len(pth) == len(w.tensors) - 1                       # the tied positional embedding has one key there
    for k in ("image_encoder.blocks.1.norm2.bias", "image_encoder.patch_embed.proj.weight", "image_encoder.neck.3.bias",
              "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "prompt_encoder.point_embeddings.3.weight",
              "prompt_encoder.mask_downscaling.6.bias", "mask_decoder.transformer.layers.1.norm4.weight",
              "mask_decoder.output_upscaling.3.bias", "mask_decoder.output_hypernetworks_mlps.2.layers.1.weight",
              "mask_decoder.iou_prediction_head.layers.2.bias", "mask_decoder.transformer.norm_final_attn.weight"):
        assert k in pth, k
    assert all(S.pth_to_hf(k) in w.tensors for k in pth)
    torch.save(pth, str(tmp_path / "sam.pth"))
    b = S.load_sam_weights(str(tmp_path / "sam.pth"))
    assert b.config == w.config and all(torch.equal(b.tensors[k], w.tensors[k]) for k in w.tensors)
    # an unknown key raises, a missing key raises
    torch.save(dict(pth, **{"image_encoder.neck.5.weight": torch.zeros(1)}), str(tmp_path / "extra.pth"))
    with pytest.raises(KeyError, match="no place"):
        S.load_sam_weights(str(tmp_path / "extra.pth"))
    torch.save(dict(pth, **{"mask_decoder.something.weight": torch.zeros(1)}), str(tmp_path / "extra2.pth"))
    with pytest.raises(KeyError, match="no place"):
        S.load_sam_weights(str(tmp_path / "extra2.pth"))
    torch.save({k: v for k, v in pth.items() if k != "mask_decoder.iou_token.weight"}, str(tmp_path / "short.pth"))
    with pytest.raises(KeyError, match="not filled"):
        S.load_sam_weights(str(tmp_path / "short.pth"))
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        S.load_sam_weights("facebook/sam-vit-huge")


def test_presets():
    h, l, b = (S.SamConfig.preset(m) for m in ("vit_h", "vit_l", "vit_b"))
    assert (h.hidden_size, h.num_hidden_layers, h.head_dim, h.windows().count(0)) == (1280, 32, 80, 4) and h == S.SamConfig()
    assert (l.hidden_size, l.num_hidden_layers, l.head_dim) == (1024, 24, 64) and (b.hidden_size, b.head_dim) == (768, 64)
    assert h.windows()[7] == 0 and h.windows()[6] == 14


def test_point_grid_and_its_order():
    p = S.point_grid(4, (84, 112))
    assert p.shape == (16, 2) and p.dtype == torch.float32
    assert torch.allclose(p[0], torch.tensor([14.0, 10.5])) and torch.allclose(p[1], torch.tensor([42.0, 10.5]))        # x fastest
    assert torch.allclose(p[4], torch.tensor([14.0, 31.5])) and torch.allclose(p[15], torch.tensor([98.0, 73.5]))


@pytest.mark.parametrize("w,h,input_size,mask_size", [(1600, 1200, (768, 1024), (768, 1024)), (1237, 822, (680, 1024), (680, 1024)),
                                                      (640, 480, (768, 1024), (480, 640))])
def test_preprocess_sizes_and_zero_padding(w, h, input_size, mask_size):
    img = np.random.default_rng(w).integers(1, 255, (h, w, 3), dtype=np.uint8)
    x, got_in, got_mask = S.preprocess(img, 1024)
    assert x.shape == (3, 1024, 1024) and x.dtype == torch.float32 and got_in == input_size and got_mask == mask_size
    assert (x[:, input_size[0]:, :] == 0).all() and (x[:, :, input_size[1]:] == 0).all()
    assert (x[:, :input_size[0], :input_size[1]] != 0).any()
    lo, hi = (0 - 123.675) / 58.395, (255 - 103.53) / 57.375
    assert float(x.min()) >= lo - 1e-5 and float(x.max()) <= hi + 1e-5


def test_select_host_pieces_against_transformers():
    from transformers.models.sam.image_processing_pil_sam import _batched_mask_to_box, _compute_stability_score
    logits = SC.mask_logits(40, 120, 160)
    v = S.upsample_host(logits, (120, 160), (120, 160))
    area, inter, union, boxes = S.mask_stats_host(v, 0.0, 1.0)
    stab = inter.float() / union.float()
    want = _compute_stability_score(v, 0.0, 1.0)
    ok = union > 0
    assert torch.equal(stab[ok], want[ok].float()) and int(area[0]) == 0 and int(area[1]) == 120 * 160
    assert torch.equal(boxes.long(), _batched_mask_to_box(v > 0.0).long()) and boxes[0].tolist() == [0, 0, 0, 0]
    assert boxes[1].tolist() == [0, 0, 159, 119]


@pytest.mark.parametrize("n,clustered", [(300, False), (1, False), (500, True)])
def test_nms_host_against_the_loop(n, clustered):
    boxes, scores = SC.random_boxes(n, 11 + n, clustered=clustered)
    if n > 10:
        boxes[5] = boxes[6] = torch.tensor([3.0, 3.0, 3.0, 9.0])            # zero area: NaN IoU with each other, both kept
        scores[7] = float("nan")
    keep = torch.rand(n, generator=torch.Generator().manual_seed(n)) > 0.2 if n > 1 else None
    for theta in (0.7, 0.3):
        got = S.nms_host(boxes, scores, keep, theta).tolist()
        assert got == SC.nms_loop(boxes.numpy(), scores.numpy(), None if keep is None else keep.numpy(), theta)
    if n > 10:
        both = S.nms_host(boxes, scores, None, 0.7).tolist()
        assert 5 in both and 6 in both and 7 not in both


def test_sam_host_equals_the_encoder_called_directly():
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    w, x = SC.weights("E1"), SC.pixels("E1")
    model = SamVisionEncoder(w.config.to_hf().vision_config)
    model.load_state_dict({k[len(S.VISION):]: t.float() for k, t in w.tensors.items()}, strict=True)
    with torch.no_grad():
        want = model.double().eval()(x[None].double()).last_hidden_state[0]
    got = S.sam_host(w, x, torch.float64, "cpu")
    assert got.shape == (64, 7, 7) and torch.equal(got, want) and float(want.abs().max()) > 0.5


def test_generator_refuses_weights_without_a_decoder():
    with pytest.raises(ValueError, match="decoder"):
        S.SamMaskGenerator(SC.weights("E1"), device="cpu", host=True)
    with pytest.raises(ValueError, match="256"):
        S.random_sam_weights(SC.config("E1", 64), decoder=True)
