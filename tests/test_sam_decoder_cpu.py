"""What the SAM decoder needs on the host: the weight table against the header's enum, the bars of the whole-decoder cases and
the conditions that keep them honest, decode_host against transformers' modules called directly, and the generator's new
keyword.  Cases, twins and bars are in tests/sam_decoder_cases.py."""
import os
import re

import pytest
import torch

import sam_decoder_cases as DC
from gaussmart_amd import _lib
from gaussmart_amd import sam as S


def test_decoder_table_follows_the_header_enum():
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    with open(os.path.join(root, "include", "gsr.h")) as f:
        text = f.read()
    assert "#define GSR_ABI_VERSION 18" in text                      # additions only
    layer = {m.group(1): int(m.group(2)) for m in re.finditer(r"GSR_SAMD_(L_[A-Z0-9]+|W_PER_LAYER) = (\d+)", text)}
    assert layer == {"L_SELF": 0, "L_NORM1": 8, "L_T2I": 10, "L_NORM2": 18, "L_MLP": 20, "L_NORM3": 24, "L_NORM4": 26, "L_I2T": 28,
                     "W_PER_LAYER": 36}
    first = {"L_SELF": "self_attn.q_proj.weight", "L_NORM1": "layer_norm1.weight", "L_T2I": "cross_attn_token_to_image.q_proj.weight",
             "L_NORM2": "layer_norm2.weight", "L_MLP": "mlp.lin1.weight", "L_NORM3": "layer_norm3.weight", "L_NORM4": "layer_norm4.weight",
             "L_I2T": "cross_attn_image_to_token.q_proj.weight"}
    for key, name in first.items():
        assert S.DEC_LAYER[layer[key]] == name
    assert len(S.DEC_LAYER) == layer["W_PER_LAYER"] == _lib.GSR_SAMD_W_PER_LAYER
    head = re.search(r"enum \{ (GSR_SAMD_W_GAUSS = 0.*?) \};", text, re.S).group(1)
    assert len(head.split(",")) - 1 == len(S.DEC_HEAD) == _lib.GSR_SAMD_W_LAYER0
    assert (_lib.GSR_SAMD_W_FINAL, _lib.GSR_SAMD_W_UP, _lib.GSR_SAMD_W_HYPER, _lib.GSR_SAMD_W_IOU, _lib.GSR_SAMD_W_COUNT) == (78, 88, 94, 112, 118)
    for line in ("GSR_SAMD_W_FINAL = GSR_SAMD_W_LAYER0 + 2 * GSR_SAMD_W_PER_LAYER", "GSR_SAMD_W_UP = GSR_SAMD_W_FINAL + 10",
                 "GSR_SAMD_W_HYPER = GSR_SAMD_W_UP + 6", "GSR_SAMD_W_IOU = GSR_SAMD_W_HYPER + 18", "GSR_SAMD_W_COUNT = GSR_SAMD_W_IOU + 6"):
        assert line in text
    w = DC.weights("D1")
    table = w.decoder_table()
    assert len(table) == _lib.GSR_SAMD_W_COUNT
    assert table[0].dtype == torch.float32 and tuple(table[0].shape) == (2, 128)
    assert torch.equal(table[0], w.tensors["prompt_encoder.shared_embedding.positional_embedding"])
    assert all(t.dtype == torch.float16 and t.is_contiguous() for t in table[1:])
    up = _lib.GSR_SAMD_W_UP
    assert [tuple(t.shape) for t in table[up:up + 6]] == [(256, 256), (256,), (64,), (64,), (128, 64), (128,)]
    c1 = w.tensors["mask_decoder.upscale_conv1.weight"]                # [ci,co,dy,dx]
    assert torch.equal(table[up][(1 * 2 + 0) * 64 + 5], c1[:, 5, 1, 0].to(torch.float16))
    assert torch.equal(table[up + 1][64:128], w.tensors["mask_decoder.upscale_conv1.bias"].to(torch.float16))
    assert tuple(table[_lib.GSR_SAMD_W_IOU + 4].shape) == (4, 256) and tuple(table[_lib.GSR_SAMD_W_HYPER + 4].shape) == (32, 256)
    assert torch.equal(table[_lib.GSR_SAMD_W_HYPER], w.tensors["mask_decoder.output_hypernetworks_mlps.1.proj_in.weight"].to(torch.float16))
    assert w.tensors["mask_decoder.iou_token.weight"].dtype == torch.float32       # SamWeights keeps its fp32 tensors
    with pytest.raises(ValueError):
        DC.SC.weights("E1").decoder_table()                            # no decoder in these


@pytest.mark.parametrize("name", ["D1", "D2", "D3"])
def test_bars_of_the_whole_decoder(name):
    b = DC.model_bars(name)
    print({k: f"{v:.3e}" for k, v in b.items()})
    DC.check_bar_conditions(b)
    low, iou = DC.twin(name)
    P, g = len(DC.points(name)), DC.weights(name).config.grid
    assert low.shape == (P, 3, 4 * g, 4 * g) and iou.shape == (P, 3) and torch.isfinite(low).all()


def test_decode_host_is_the_modules_called_directly():
    w, emb, pts = DC.weights("D1"), DC.embedding("D1"), DC.points("D1")
    prompt, decoder, wide = S.host_decoder(w, torch.float32, "cpu")
    with torch.no_grad():
        sparse, dense = prompt(pts[None, :, None, :], torch.ones(1, len(pts), 1, dtype=torch.int64), None, None)
        m, q = decoder(image_embeddings=emb, image_positional_embeddings=wide, sparse_prompt_embeddings=sparse,
                       dense_prompt_embeddings=dense, multimask_output=True)
    low, iou = S.decode_host(w, emb, None, pts, torch.float32, "cpu")
    assert torch.equal(low, m[0]) and torch.equal(iou, q[0])
    # batches of 4 give the rows of one batch
    low4, iou4 = S.decode_host(w, emb, wide, pts, torch.float32, "cpu", points_per_batch=4)
    assert torch.allclose(low4, low, atol=1e-5) and torch.allclose(iou4, iou, atol=1e-5)


def test_generator_keyword():
    w = DC.weights("D1")
    gen = S.SamMaskGenerator(w, device="cpu", host=True)
    assert gen.decoder == "torch"
    with pytest.raises(ValueError, match="host=True"):
        S.SamMaskGenerator(w, device="cpu", host=True, decoder="hip")
    with pytest.raises(ValueError, match="not 'torch' or 'hip'"):
        S.SamMaskGenerator(w, device="cpu", host=True, decoder="triton")
    # the host generator's decode is decode_host in fp32
    low, iou = gen.decode(DC.embedding("D1"), DC.points("D1"))
    want = S.decode_host(w, DC.embedding("D1"), None, DC.points("D1"), torch.float32, "cpu")
    assert torch.equal(low, want[0]) and torch.equal(iou, want[1])
