"""gaussmart_amd.sam2 without a GPU: the configuration, its JSON and its refusals, the weights on disk (video-memory keys
included), the weight table (padded patch rows, the position table against transformers' _get_pos_embed, the neck's order),
preprocess2 and the point grid, the one-step selection twin against a plain F.interpolate loop (and against SAM's two-step
route, which must differ), and the bar conditions of the whole-encoder test.  Cases and twins are in tests/sam2_cases.py."""
import numpy as np
import pytest
import torch

import sam2_cases as SC
from gaussmart_amd import _lib
from gaussmart_amd import sam as S1
from gaussmart_amd import sam2 as S2


def test_config_defaults_presets_and_json_round_trip():
    c = S2.Sam2Config()
    assert (c.embed_dim, c.num_heads, c.blocks_per_stage, c.global_attention_blocks) == (144, 2, (2, 6, 36, 4), (23, 33, 43))
    assert (c.window_size_per_stage, c.background_size, c.fpn_hidden_size, c.fpn_top_down_levels, c.image_size) == ((8, 4, 16, 8), (7, 7), 256, (2, 3), 1024)
    assert c.head_dim == 72 and c.dims() == [144, 288, 576, 1152] and c.heads() == [2, 4, 8, 16] and c.grids() == [256, 128, 64, 32]
    assert S2.Sam2Config.preset("large") == c.check()
    for name, embed, heads, blocks, glob, hd in (("tiny", 96, 1, (1, 2, 7, 2), (5, 7, 9), 96), ("small", 96, 1, (1, 2, 11, 2), (7, 10, 13), 96),
                                                 ("base_plus", 112, 2, (2, 3, 16, 3), (12, 16, 20), 56)):
        p = S2.Sam2Config.preset(name)
        assert (p.embed_dim, p.num_heads, p.blocks_per_stage, p.global_attention_blocks, p.head_dim) == (embed, heads, blocks, glob, hd)
        assert S2.Sam2Config.from_json(p.to_json()) == p
        with pytest.raises(ValueError, match="not a multiple of the window 14"):     # their windows need Hiera's padding
            p.check()
    assert S2.Sam2Config.preset("base_plus").background_size == (14, 14)
    with pytest.raises(ValueError):
        S2.Sam2Config.preset("huge")
    for name in SC.ENCODER_CASES:
        cfg = SC.config(name)
        assert S2.Sam2Config.from_json(cfg.to_json()) == cfg
        hf = cfg.to_hf()            # transformers reads the same numbers back
        b = hf.vision_config.backbone_config
        assert list(b.embed_dim_per_stage) == cfg.dims() and list(b.blocks_per_stage) == list(cfg.blocks_per_stage)
        assert list(hf.vision_config.backbone_channel_list) == cfg.dims()[::-1]
    # a block plan: (stage, start, grid, window, stride); a stage start runs on the previous grid with the previous window
    plan = SC.config("H1").block_plan()
    assert plan == [(0, False, 64, 8, 1), (1, True, 64, 8, 2), (1, False, 32, 4, 1), (2, True, 32, 4, 2), (2, False, 16, 0, 1),
                    (2, False, 16, 16, 1), (3, True, 16, 16, 2), (3, False, 8, 8, 1)]


def test_every_refusal_of_the_config_check():
    base = dict(embed_dim=144, num_heads=2, blocks_per_stage=(1, 2, 3, 2), global_attention_blocks=(4,), image_size=256)
    S2.Sam2Config(**base).check()
    for kw, err in ((dict(image_size=128), ValueError),                     # the last grid 4 is no multiple of the window 8
                    (dict(image_size=224), ValueError),
                    (dict(query_stride=(1, 1)), ValueError),
                    (dict(query_stride=(2, 1)), ValueError),
                    (dict(global_attention_blocks=(3,)), ValueError),       # block 3 starts stage 2
                    (dict(embed_dim=100), NotImplementedError),             # head_dim 50
                    (dict(embed_dim=96, num_heads=2), NotImplementedError), # head_dim 48
                    (dict(embed_dim=145), ValueError),
                    (dict(window_size_per_stage=(8, 4, 14, 7)), ValueError),
                    (dict(window_size_per_stage=(8, 3, 16, 8)), ValueError),    # 32 % 3, and an odd window under a stride of 2
                    (dict(blocks_per_stage=(1, 2, 3)), ValueError),
                    (dict(blocks_per_stage=(1, 0, 3, 2)), ValueError),
                    (dict(fpn_hidden_size=100), ValueError),
                    (dict(fpn_top_down_levels=(2, 4)), ValueError),
                    (dict(layer_norm_eps=1e-5), ValueError)):
        with pytest.raises(err):
            S2.Sam2Config(**{**base, **kw}).check()
    # a stage that does not double its width can only come from a file
    d = S2.Sam2Config(**base).to_json()
    d["vision_config"]["backbone_config"]["embed_dim_per_stage"] = [144, 288, 576, 1000]
    with pytest.raises(ValueError, match="double"):
        S2.Sam2Config.from_json(d)
    d = S2.Sam2Config(**base).to_json()
    d["vision_config"]["backbone_config"]["patch_stride"] = [8, 8]
    with pytest.raises(NotImplementedError):
        S2.Sam2Config.from_json(d)
    with pytest.raises(NotImplementedError, match="decoder='hip'"):
        S2.Sam2MaskGenerator(SC.weights("H2"), decoder="hip", host=True, device="cpu")


def test_weights_save_load_and_refusals(tmp_path):
    w = SC.weights("H2")
    S2.save_sam2_weights(w, str(tmp_path / "ckpt"))
    a = S2.load_sam2_weights(str(tmp_path / "ckpt"))
    assert a.config == w.config and a.tensors.keys() == w.tensors.keys()
    assert all(torch.equal(a.tensors[k], w.tensors[k]) and a.tensors[k].dtype == w.tensors[k].dtype for k in w.tensors)
    assert w.tensors[S2.BACKBONE + "blocks.0.attn.qkv.weight"].dtype == torch.float16 and w.tensors[S2.CONV_S[0]].dtype == torch.float16
    assert w.tensors[S2.NO_MEMORY].dtype == torch.float32 and w.tensors["mask_decoder.iou_token.weight"].dtype == torch.float32
    # the keys of a video checkpoint that transformers itself ignores are dropped; anything else without a place raises
    video = dict(w.tensors)
    video.update({"memory_encoder.projection.weight": torch.zeros(2), "mask_downsample.weight": torch.zeros(2), "no_object_pointer": torch.zeros(2),
                  "memory_attention.layers.0.self_attn.q_proj.weight": torch.zeros(2), "object_pointer_proj.proj_in.bias": torch.zeros(2),
                  "occlusion_spatial_embedding_parameter": torch.zeros(2), "no_memory_positional_encoding": torch.zeros(2),
                  "temporal_positional_encoding_projection_layer.weight": torch.zeros(2)})
    b = S2.Sam2Weights(w.config, video)
    assert b.tensors.keys() == w.tensors.keys()
    with pytest.raises(KeyError, match="no place"):
        S2.Sam2Weights(w.config, {**w.tensors, "vision_encoder.backbone.blocks.9.proj.weight": torch.zeros(2)})
    short = dict(w.tensors)
    del short[S2.NO_MEMORY]
    with pytest.raises(KeyError, match="not filled"):
        S2.Sam2Weights(w.config, short)
    with pytest.raises(ValueError, match="must be"):
        S2.Sam2Weights(w.config, {**w.tensors, S2.BACKBONE + "pos_embed": torch.zeros(1, 96, 8, 8)})
    with pytest.raises(FileNotFoundError):
        S2.load_sam2_weights(str(tmp_path / "nothing.pt"))
    # the random recipe fills what default initialisation zeroes
    for k in (S2.BACKBONE + "pos_embed", S2.BACKBONE + "pos_embed_window", S2.NO_MEMORY):
        assert float(w.tensors[k].float().std()) > 0.5


@pytest.mark.parametrize("name", ["H1", "H2"])
def test_weight_table(name):
    w, cfg = SC.weights(name), SC.config(name)
    tab = w.table()
    assert len(tab) == _lib.GSR_SAM2_W_BLOCK0 + _lib.GSR_SAM2_W_PER_BLOCK * cfg.total_blocks + _lib.GSR_SAM2_W_NECK == 3 + 14 * cfg.total_blocks + 13
    model = S2.host_model(w, torch.float64)
    # the patch rows: 147 columns in Conv2d's own order and 5 zeros; the product over 152 is the convolution
    pw = tab[0]
    assert pw.shape == (cfg.embed_dim, 152) and pw.dtype == torch.float16 and not pw[:, 147:].any()
    x = SC.pixels(name)[None].double()
    conv = model.vision_encoder.backbone.patch_embed.projection(x)[0]                     # [embed,64,64]
    cols = torch.nn.functional.unfold(x, 7, padding=3, stride=4)[0].T                     # [T,147], k = c 49 + ky 7 + kx
    mine = torch.nn.functional.pad(cols, (0, 5)) @ pw.double().T + tab[1].double()
    assert torch.allclose(mine.T.reshape_as(conv), conv, atol=1e-12)
    # the position table: _get_pos_embed in fp64, against the fp32 computation rounded once to fp16
    ref = model.vision_encoder.backbone._get_pos_embed((64, 64))[0]
    assert tab[2].shape == (64, 64, cfg.embed_dim) and tab[2].dtype == torch.float16
    ref = ref.detach()
    assert float((tab[2].double() - ref).abs().max()) <= 2.0 ** -11 * float(ref.abs().max()) + 1e-5
    # both tables show in it
    assert float(ref.std()) > 1.0
    # the blocks: a projection only where a stage starts
    starts = [p[1] for p in cfg.block_plan()]
    for b, start in enumerate(starts):
        row = tab[3 + 14 * b:3 + 14 * (b + 1)]
        assert all(t is not None and t.dtype == torch.float16 for t in row[:12]) and (row[12] is not None) == start == (row[13] is not None)
    # the neck: convs[3 - i] takes stage i, then conv_s0, conv_s1, no_memory_embedding in fp32
    neck = tab[-13:]
    assert [tuple(t.shape) for t in neck[0:8:2]] == [(256, d) for d in cfg.dims()] and [tuple(t.shape) for t in neck[8:]] == [(32, 256), (32,), (64, 256), (64,), (256,)]
    assert torch.equal(neck[0], w.tensors["vision_encoder.neck.convs.3.weight"].reshape(256, -1)) and neck[12].dtype == torch.float32


def test_preprocess2_and_the_grid():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)
    x, input_size, mask_size = S2.preprocess2(img, 256)
    assert x.shape == (3, 256, 256) and x.dtype == torch.float32 and input_size == (256, 256) and mask_size == (96, 128)
    big = rng.integers(0, 256, (1500, 2000, 3), dtype=np.uint8)
    assert S2.preprocess2(big, 64)[1:] == ((64, 64), (768, 1024))              # the reference's first resize decides the mask size
    # no resize when the picture already has the size: the values are the pixels / 255, normalised
    sq = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    y = S2.preprocess2(sq, 32)[0]
    want = (torch.from_numpy(sq).permute(2, 0, 1).float() / 255 - torch.tensor(S2.IMAGE_MEAN).view(3, 1, 1)) / torch.tensor(S2.IMAGE_STD).view(3, 1, 1)
    assert torch.allclose(y, want, atol=1e-6)
    pts = S1.point_grid(4, input_size)
    assert pts.shape == (16, 2) and pts[0].tolist() == [32.0, 32.0] and pts[1].tolist() == [96.0, 32.0] and pts[-1].tolist() == [224.0, 224.0]


@pytest.mark.parametrize("Lr,cone_size,mask_size,n", SC.MASK_SHAPES[:3])
def test_select_host_one_step_against_a_plain_loop(Lr, cone_size, mask_size, n):
    logits = SC.mask_logits(Lr, *cone_size, n=n)
    planes = SC.interpolate_loop(logits, mask_size)
    assert torch.equal(S1.upsample_host(logits, None, mask_size, direct=True), planes)
    g = torch.Generator().manual_seed(Lr)
    iou = torch.rand(n, generator=g)
    sel = S1.select_host(logits[:, None], iou[:, None], None, mask_size, pred_iou_thresh=0.3, stability_score_thresh=0.5, box_nms_thresh=1.0,
                         direct=True)
    area, inter, union, boxes = S1.mask_stats_host(planes)
    keep = (iou > 0.3) & (inter.float() / union.float() >= 0.5)
    assert torch.equal(sel["keep_in"], keep) and 0 < int(keep.sum()) < n
    order = torch.nonzero(keep).reshape(-1)
    order = order[torch.sort(iou[order], descending=True, stable=True).indices]
    assert torch.equal(sel["index"], order) and torch.equal(sel["masks"].bool(), planes[order] > 0)
    assert torch.equal(sel["area"], area[order]) and torch.equal(sel["boxes"], boxes[order])


@pytest.mark.parametrize("k", [0, 3])
def test_the_two_step_route_flips_decided_pixels(k):
    """Reusing SAM's L -> 4 L -> resize for SAM2 (the whole 4 L frame as the input size: SAM2 has no padding to crop) cannot
    pass the GPU test: it disagrees with the one-step truth on pixels that truth decides."""
    Lr, cone_size, mask_size, n = SC.MASK_SHAPES[k]
    logits = SC.mask_logits(Lr, *cone_size, n=n)
    one, two = SC.mask_truth(logits, mask_size), SC.mask_truth(logits, mask_size, two_step=(4 * Lr, 4 * Lr))
    flips = int(((one["on"] != two["on"]) & one["decided"]).sum())
    share = float((~one["decided"]).sum()) / one["decided"].numel()
    print(f"L{Lr} -> {mask_size}: the two-step route flips {flips} decided pixels; undecided share {share:.2e}")
    assert flips >= 1 and share <= 1e-3


@pytest.mark.parametrize("name", ["H1", "H2"])
def test_bar_conditions(name):
    bars, moves = SC.model_bars(name), SC.wrong_moves(name)
    print(SC.bars_line(name, bars, moves))
    SC.check_bar_conditions(bars, moves)
    o = SC.twin(name)
    assert [tuple(m.shape) for m in o] == [(32, 64, 64), (64, 32, 32), (256, 16, 16)]
    # what each wrong reading can and cannot reach: the top-down path only feeds level 2
    assert moves[0]["no_top_down"] == 0 and moves[1]["no_top_down"] == 0 and moves[2]["no_top_down"] > 10 * bars[2]["bar"]


def test_attention64_against_transformers_attention():
    """tests/sam2_cases.attention64 (the GPU test's reference) against Sam2MultiScaleAttention itself, windows partitioned by
    transformers' own helper, with and without the query pooling."""
    from transformers.models.sam2 import modeling_sam2 as M
    cfg = SC.config("H1").to_hf().vision_config.backbone_config
    for g, w, stride, heads, hd in ((16, 8, 1, 2, 72), (16, 4, 2, 2, 96), (16, 0, 1, 4, 72)):
        dim = heads * hd
        attn = M.Sam2MultiScaleAttention(cfg, dim, dim, heads, query_stride=(2, 2) if stride == 2 else None).double().eval()
        gen = torch.Generator().manual_seed(g + w + hd)
        qkv = torch.randn(g * g, 3 * dim, generator=gen).to(torch.float16)
        with torch.no_grad():
            attn.proj.weight.copy_(torch.eye(dim))
            attn.proj.bias.zero_()
            attn.qkv = torch.nn.Identity()          # the module's input IS the test's qkv
            x = qkv.double().reshape(1, g, g, 3 * dim)
            s = w or g
            if w:
                x, pad = M.window_partition(x, w)
            y = attn(x)
            if w:
                y = M.window_unpartition(y, s // stride, (g // stride, g // stride), (g // stride, g // stride))
        want, bar = SC.attention64(qkv, g, w, stride, heads, hd)
        # transformers' eager attention takes its softmax in fp32 whatever the model's dtype: 2^-24 on weights below 1
        assert float((y.reshape(-1, dim) - want).abs().max()) < 2e-6 and float(bar.max()) < 2e-2
