"""SAM2's prompt encoder and mask decoder without a device: the weight table of gsr_sam2_decode against include/gsr.h, the
bars of the whole-decoder cases and their conditions, decode_host2 against the modules called one by one, and the generator's
decoder keyword.  Cases, twins and bars are in tests/sam2_decoder_cases.py."""
import os
import re

import pytest
import torch

import sam2_decoder_cases as KC
from gaussmart_amd import _lib
from gaussmart_amd import sam2 as S2

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsr.h")


def test_decoder_table_against_the_header():
    with open(HEADER) as f:
        text = f.read()
    assert "#define GSR_ABI_VERSION 18" in text
    assert re.search(r"GSR_SAM2D_W_OBJ_TOKEN = GSR_SAMD_W_COUNT, GSR_SAM2D_W_COUNT = GSR_SAMD_W_COUNT \+ 1", text)
    assert (_lib.GSR_SAMD_W_COUNT, _lib.GSR_SAM2D_W_OBJ_TOKEN, _lib.GSR_SAM2D_W_COUNT) == (118, 118, 119)
    for name in ("gsr_sam2_dec_t2i", "gsr_sam2_dec_i2t_workspace_bytes", "gsr_sam2_dec_i2t", "gsr_sam2_dec_upscale_workspace_bytes",
                 "gsr_sam2_dec_upscale", "gsr_sam2_dec_num_weights", "gsr_sam2_decode_workspace_bytes", "gsr_sam2_decode"):
        assert re.search(r"\b%s\(" % name, text), name
    w = KC.weights("K1")
    t, table = w.tensors, w.decoder_table()
    assert len(table) == 119
    assert table[0].dtype == torch.float32 and torch.equal(table[0], t["prompt_encoder.shared_embedding.positional_embedding"])
    assert all(x.dtype == torch.float16 for x in table[1:]) and all(x.is_contiguous() for x in table)
    # Sam2Weights.tensors keeps its fp32 decoder tensors
    assert t["mask_decoder.iou_token.weight"].dtype == torch.float32 and t[S2.OBJ_TOKEN].dtype == torch.float32
    md, l1 = "mask_decoder.", _lib.GSR_SAMD_W_LAYER0 + _lib.GSR_SAMD_W_PER_LAYER

    def same(i, key):
        return torch.equal(table[i].float(), t[key].reshape(table[i].shape))        # random weights are fp16 values already
    assert table[_lib.GSR_SAMD_W_POINT1].shape == (1, 256) and torch.equal(table[1].float(), t["prompt_encoder.point_embed.weight"][1:2])
    assert not torch.equal(table[1].float(), t["prompt_encoder.point_embed.weight"][0:1])
    assert same(2, "prompt_encoder.not_a_point_embed.weight") and same(3, "prompt_encoder.no_mask_embed.weight")
    assert same(4, md + "iou_token.weight") and same(5, md + "mask_tokens.weight") and table[5].shape == (4, 256)
    assert same(_lib.GSR_SAMD_W_LAYER0 + 6, md + "transformer.layers.0.self_attn.o_proj.weight")
    assert same(l1 + 10 + 6, md + "transformer.layers.1.cross_attn_token_to_image.o_proj.weight") and table[l1 + 16].shape == (256, 128)
    assert same(l1 + 20, md + "transformer.layers.1.mlp.proj_in.weight") and table[l1 + 20].shape == (2048, 256)
    assert same(l1 + 22, md + "transformer.layers.1.mlp.proj_out.weight") and table[l1 + 22].shape == (256, 2048)
    assert same(l1 + 26, md + "transformer.layers.1.layer_norm4.weight")
    assert same(l1 + 28 + 7, md + "transformer.layers.1.cross_attn_image_to_token.o_proj.bias")
    assert same(_lib.GSR_SAMD_W_FINAL + 6, md + "transformer.final_attn_token_to_image.o_proj.weight")
    assert same(_lib.GSR_SAMD_W_FINAL + 8, md + "transformer.layer_norm_final_attn.weight")
    assert same(_lib.GSR_SAMD_W_HYPER, md + "output_hypernetworks_mlps.1.proj_in.weight")
    assert same(_lib.GSR_SAMD_W_IOU + 4, md + "iou_prediction_head.proj_out.weight") and table[_lib.GSR_SAMD_W_IOU + 4].shape == (4, 256)
    assert same(_lib.GSR_SAM2D_W_OBJ_TOKEN, S2.OBJ_TOKEN) and table[118].shape == (1, 256)
    # the transposed convolutions: row (dy 2 + dx) co_n + co, column ci; the biases once per tap
    up = _lib.GSR_SAMD_W_UP
    c1, c2 = t[md + "upscale_conv1.weight"], t[md + "upscale_conv2.weight"]
    assert table[up].shape == (256, 256) and table[up + 4].shape == (128, 64)
    for dy, dx, co, ci in ((0, 0, 0, 0), (0, 1, 5, 17), (1, 0, 63, 255), (1, 1, 31, 100)):
        assert float(table[up][(dy * 2 + dx) * 64 + co, ci]) == float(c1[ci, co, dy, dx])
        assert float(table[up + 4][(dy * 2 + dx) * 32 + co % 32, ci % 64]) == float(c2[ci % 64, co % 32, dy, dx])
    assert torch.equal(table[up + 1].float(), t[md + "upscale_conv1.bias"].repeat(4)) and table[up + 5].shape == (128,)
    assert same(up + 2, md + "upscale_layer_norm.weight")


@pytest.mark.parametrize("name", ["K1", "K2"])
def test_bar_conditions(name):
    b = KC.model_bars(name)
    print(KC.bars_line(name, b))
    KC.check_bar_conditions(b)
    w = KC.weights(name)
    w.config.check()
    g = w.config.image_size // 16
    low, iou = KC.twin(name)
    n = KC.DECODER_CASES[name][3]
    assert low.shape == (n, 3, 4 * g, 4 * g) and iou.shape == (n, 3) and len(KC.points(name)) == n
    assert 0.0 < float(iou.min()) and float(iou.max()) < 1.0            # the sigmoid's range, not saturated


def test_decode_host2_against_the_modules():
    """decode_host2 (points_per_batch at a time, through Sam2MaskDecoder.forward) against the prompt encoder and the decoder's
    parts called one by one on all points at once: the same function, so fp64 agrees to rounding."""
    w, m, pts = KC.weights("K1"), KC.maps("K1"), KC.points("K1")
    modules = S2.host_decoder2(w, torch.float64, "cpu")
    low, iou = S2.decode_host2(w, list(m), pts, torch.float64, "cpu", modules, points_per_batch=4)
    low_d, iou_d = KC.modules_direct(modules, m, pts, torch.float64)
    assert low.shape == low_d.shape and float((low - low_d).abs().max()) < 1e-10 and float((iou - iou_d).abs().max()) < 1e-12
    # the batching changes nothing, and the seven-token reading is a different function
    low1, iou1 = S2.decode_host2(w, list(m), pts, torch.float64, "cpu", modules, points_per_batch=64)
    assert float((low - low1).abs().max()) < 1e-10 and float((iou - iou1).abs().max()) < 1e-12
    low7, _ = KC.modules_direct(modules, m, pts, torch.float64, obj_token=False)
    assert float((low7 - low).abs().max()) > 0.1


def test_generator_decoder_keyword():
    w = KC.weights("K1")
    with pytest.raises(NotImplementedError, match="decoder='hip'"):
        S2.Sam2MaskGenerator(w, decoder="hip", host=True, device="cpu")
    with pytest.raises(ValueError):
        S2.Sam2MaskGenerator(w, device="cpu", decoder="triton")
    gen = S2.Sam2MaskGenerator(w, device="cpu", decoder="hip")          # constructs without touching a device
    assert gen.decoder == "hip" and gen._hip is None and gen._modules is None
    assert S2.Sam2MaskGenerator(w, device="cpu").decoder == "torch"
