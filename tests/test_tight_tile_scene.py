"""The scenes of tests/test_gpu_tight_tiles.py hold what that file says they hold, checked without a GPU with the float32
transcription of preprocess_fwd's two boxes in scripts/tight_tile_count.py."""
import os
import sys

import pytest
import torch

from test_gpu_tight_tiles import SIZES, THIN, FULL, GRAZING, EDGES, FAINT, build_scene

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))


@pytest.mark.parametrize("w,h,seed", SIZES)
def test_constructed_cases(w, h, seed):
    from tight_tile_count import tile_rects, count_per
    p, cam = build_scene(w, h, seed)
    r = tile_rects(p, cam, w, h)
    gx, gy = (w + 15) // 16, (h + 15) // 16
    ref, tight, radii = count_per(r["ref"]), count_per(r["tight"]), r["radii"]
    size = lambda rect, i: (int(rect[2][i] - rect[0][i]), int(rect[3][i] - rect[1][i]))
    assert size(r["ref"], THIN) == (3, 3) and size(r["tight"], THIN) == (3, 1)
    faint = torch.tensor(FAINT)
    seen = faint[radii[faint] > 0]
    assert seen.numel() > 0 and bool((ref[seen] > 0).all()) and bool((tight[seen] == 0).all())
    assert int(r["box"][0][GRAZING]) == -32768 and int(r["box"][1][GRAZING]) == 32767        # dd >= 0: never culled
    assert int(r["box"][0][FULL]) > -32768                                                   # ... unlike an ordinary large splat
    assert int(ref[GRAZING]) == int(tight[GRAZING]) > 1 and gx * gy == int(ref[FULL]) == int(tight[FULL])
    edges = torch.tensor(EDGES)
    assert bool((tight[edges] > 0).all())
    cx_out = 0
    for i in EDGES:     # the 3-sigma rect reaches the frame although the centre lies outside it
        x, y, z = p["xyz"][i].tolist()
        cx_out += int(abs(x / z) > 0.5773 or abs(y / z) > 0.5773 * h / w)
    assert cx_out == len(EDGES)
    assert bool((tight <= ref).all()) and int(tight.sum()) < int(ref.sum())
    assert int(((radii > 0) & (tight == 0)).sum()) >= seen.numel()
