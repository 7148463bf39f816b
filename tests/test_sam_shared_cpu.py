"""The Python layer of SAM and SAM2 mask generation has one body per step (gaussmart_amd/sam.py); sam2.py supplies hooks only.

  * Sam2MaskGenerator defines none of the generator's steps itself.
  * select reads from the instance only `host` and the four thresholds: a __new__ stub of either class with exactly those runs
    it (scripts/sam_bench.py and scripts/sam2_bench.py time it that way), and with host=True it is select_host, two-step for
    SAM and direct for SAM2.
  * ModelWeights.copy leaves the object it copies as it was."""
import pytest
import torch

import sam_cases as SC
from gaussmart_amd import sam as S1
from gaussmart_amd import sam2 as S2

STEPS = ("select", "_decode_hip", "_decoder_hip", "_run", "generate", "generate_device")
THRESHOLDS = dict(pred_iou_thresh=0.55, stability_score_thresh=0.8, stability_score_offset=1.0, box_nms_thresh=0.7)


def test_sam2_generator_overrides_no_step():
    assert issubclass(S2.Sam2MaskGenerator, S1.SamMaskGenerator)
    own = vars(S2.Sam2MaskGenerator)
    assert [name for name in STEPS + ("__init__",) if name in own] == []
    assert all(name in vars(S1.SamMaskGenerator) for name in STEPS)
    for name in ("decoder_table", "to", "sub", "copy"):         # one body for the weights' shared methods too
        assert getattr(S1.SamWeights, name) is getattr(S2.Sam2Weights, name) is getattr(S1.ModelWeights, name)


@pytest.mark.parametrize("cls,direct", [(S1.SamMaskGenerator, False), (S2.Sam2MaskGenerator, True)])
def test_select_of_a_stub_with_five_attributes_is_select_host(cls, direct):
    gen = torch.Generator().manual_seed(3)
    ys, xs = torch.meshgrid(torch.arange(16.0), torch.arange(16.0), indexing="ij")
    centre, radius = 4 + 8 * torch.rand(6, 2, generator=gen), 3 + 3 * torch.rand(6, generator=gen)
    dist = torch.sqrt((ys - centre[:, 0, None, None]) ** 2 + (xs - centre[:, 1, None, None]) ** 2)
    low = (8 * (radius[:, None, None] - dist) + 0.3 * torch.randn(6, 16, 16, generator=gen)).reshape(2, 3, 16, 16)     # 6 planes of logits
    iou = torch.tensor([[0.9, 0.5, 0.7], [0.6, 0.95, 0.4]])
    input_size, mask_size = (48, 64), (37, 50)      # the two-step path crops 64 x 64 to 48 x 64; the direct one does not read it
    stub = cls.__new__(cls)
    stub.host = True
    for k, v in THRESHOLDS.items():
        setattr(stub, k, v)
    assert set(vars(stub)) == {"host", *THRESHOLDS}
    got = stub.select(low, iou, input_size, mask_size)
    want = S1.select_host(low, iou, input_size, mask_size, **THRESHOLDS, direct=direct)
    other = S1.select_host(low, iou, input_size, mask_size, **THRESHOLDS, direct=not direct)
    assert set(got) == set(want) and len(want["index"]) >= 2
    for k in want:          # stability is NaN where a plane is empty (0 / 0)
        a, b = (torch.nan_to_num(t, nan=-1.0) if t.dtype.is_floating_point else t for t in (got[k], want[k]))
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert not torch.equal(got["masks"], other["masks"])      # the two resamplings differ here


def test_copy_leaves_the_original_untouched():
    w = SC.weights("E1", 256)
    names, held = list(w.tensors), dict(w.tensors)
    key = "prompt_encoder.no_mask_embed.weight"
    before = {k: t.clone() for k, t in w.tensors.items()}
    c = w.copy(replace={key: torch.zeros_like(w.tensors[key])}, keep=lambda k: not k.startswith(S1.VISION))
    assert type(c) is type(w) and c.config is w.config and c.decoder == w.decoder
    assert c.tensors is not w.tensors and not any(k.startswith(S1.VISION) for k in c.tensors) and key in c.tensors
    assert not c.tensors[key].any() and w.tensors[key].any()
    assert list(w.tensors) == names and all(w.tensors[k] is held[k] and torch.equal(w.tensors[k], before[k]) for k in names)
    moved = w.to("cpu")
    assert moved is not w and moved.tensors is not w.tensors and list(moved.tensors) == names
