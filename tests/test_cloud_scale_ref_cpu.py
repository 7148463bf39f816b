"""The vectorised references of tests/cloud_scale_ref.py equal the scalar restatements bit for bit on every down-sampling and
voxel-grid fixture of the GPU modules, so a large case that fails in tests/test_gpu_cloud_scale.py cannot be the fast
reference's doing."""
import numpy as np
import pytest

import cloud_scale_ref as F
import mesh_eval_ref as ME
import tnt_eval_ref as TN


@pytest.mark.parametrize("name", list(ME.DOWNSAMPLE))
def test_greedy_keep_fast_equals_scalar(name):
    make, thresh, _ = ME.DOWNSAMPLE[name]
    pts = make()
    want = ME.cached(("keep", name), lambda: ME.greedy_keep(pts, thresh))
    got = F.greedy_keep_fast(pts, thresh)
    assert got.dtype == bool and got.shape == (len(pts),) and np.array_equal(got, want)
    if len(pts) > 1:
        assert name == "duplicates_200" or 1 < want.sum() < len(pts)          # the fixtures decide something


def test_greedy_keep_fast_ties_at_the_threshold():
    """pairs exactly at thresh (dyadic lattice) are neighbours, pairs one ulp beyond are not: the filter is EVAL_DIST's `<=`"""
    line = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [np.nextafter(np.float32(0.75), np.float32(1)), 0, 0]], np.float32)
    assert F.greedy_keep_fast(line, 0.25).tolist() == [True, False, True, True] == ME.greedy_keep(line, 0.25).tolist()


@pytest.mark.parametrize("name", list(TN.VOXEL))
def test_voxel_fast_equals_scalar(name):
    make, size = TN.VOXEL[name]
    pts = make()
    want, row = TN.voxel(pts, size)
    got, grow = F.voxel_fast(pts, size)
    assert got.dtype == np.float32 and grow.dtype == np.int32
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(grow, row)


def test_voxel_fast_refuses_like_the_scalar_one():
    pts = TN.cloud(300, 66)
    for fn in (TN.voxel, F.voxel_fast):
        with pytest.raises(ValueError, match="voxel_size"):
            fn(pts, 1e-6)


def test_voxel_fast_sums_in_input_order():
    """one cell whose float64 sum depends on the order (+-2^40 between values in [1, 2)): the sequential order is the rule, the
    fast reference keeps it, and numpy's pairwise sum of the same column gives another float32 point"""
    k = 3000
    small = np.random.default_rng(0).random((2 * k, 3)).astype(np.float32) + 1
    pts = np.empty((4 * k, 3), np.float32)
    pts[0::4], pts[1::4], pts[2::4], pts[3::4] = np.float32(2.0 ** 40), small[:k], -np.float32(2.0 ** 40), small[k:]
    want, _ = TN.voxel(pts, 2.0 ** 43)
    got, row = F.voxel_fast(pts, 2.0 ** 43)
    assert len(want) == 1 and not row.any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    pairwise = np.array([np.ascontiguousarray(pts[:, a].astype(np.float64)).sum() / len(pts) for a in range(3)]).astype(np.float32)
    assert (pairwise.view(np.uint32) != want.view(np.uint32)).all()


@pytest.mark.parametrize("n", [0, 1, 255, 257, 4099, 262145 + 513])
def test_fixed_order_sum_equals_scalar(n):
    """the scalar statement: every thread's own loop, the tree as a loop over threads, the partials the same way"""
    x = F.wide_values(n, 7 + n)

    def tree(v):
        v, d = list(v), 128
        while d:
            for t in range(d):
                v[t] += v[t + d]
            d //= 2
        return v[0]

    def group(v, first, stride):                            # the workgroup whose thread t starts at first + t
        out = []
        for t in range(256):
            acc = 0.0
            for e in v[first + t::stride]:
                acc += e
            out.append(acc)
        return tree(out)

    v = x.tolist()
    blocks = min(1024, -(-n // 256))
    partial = [group(v, b * 256, blocks * 256) for b in range(blocks)]
    want = group(partial, 0, 256) if blocks else 0.0
    got = F.fixed_order_sum(x)
    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
    if n >= 255:
        assert got != float(np.cumsum(x)[-1])               # a sequential sum is another number: the order shows
