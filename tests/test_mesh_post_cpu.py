"""Mesh post-processing without a GPU: the fixtures of the device tests against the figures of the host post_process_mesh
(so that they cannot drift), the argument checks of the gsr_mesh_* / gsr_depth_aabb entry points (they run before any device
work), and the host-side behaviour of the Python layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_post_fixtures as Fx
from gaussmart_amd import _lib
from gaussmart_amd.mesh import DeviceTriangleMesh, TriangleMesh, post_process_mesh_device

GSR_E_INVALID, GSR_E_UNSUPPORTED = -1, -4


# ---------------------------------------------------------------- fixtures
def test_mixed_fixture_figures():
    m = Fx.mixed()
    assert len(m.vertices) == 600 and len(m.triangles) == 10 + 60 + 500 + 7
    for k, (nv, nt) in Fx.MIXED_EXPECTED.items():
        r = Fx.host_filtered("mixed", k)
        assert (len(r.vertices), len(r.triangles)) == (nv, nt), k
    labels, sizes = Fx.reference_labels(m.triangles, 600)
    # the isolated triangle; the strip of 10; the strip of 60 + three on its edge (12, 13); the strip of 500 + the duplicate
    # + the two degenerate triangles, which hang on edges (100, 101) and (200, 201)
    assert sorted(np.unique(sizes).tolist()) == [1, 10, 63, 503]
    assert (labels <= np.arange(len(labels))).all()
    r = Fx.host_filtered("mixed", 1, False)
    assert r.vertices.shape == (0, 3) and r.triangles.shape == (0, 3) and r.vertex_colors.shape == (0, 3)


def test_holed_grid_fixture_figures():
    assert len(Fx.holed_grid().triangles) == Fx.HOLED_GRID_TRIANGLES
    for k, (nv, nt) in Fx.HOLED_GRID_EXPECTED.items():
        r = Fx.host_filtered("holed_grid", k)
        assert (len(r.vertices), len(r.triangles)) == (nv, nt), k


def test_reference_labels_match_the_host_filter():
    """The scipy labels the device labels are held to give the same keep mask as post_process_mesh."""
    m = Fx.holed_grid()
    _, sizes = Fx.reference_labels(m.triangles, len(m.vertices))
    labels, _ = Fx.reference_labels(m.triangles, len(m.vertices))
    counts = np.sort(sizes[labels == np.arange(len(labels))])
    for k in (1, 3, 10, 1000):
        thr = max(counts[-min(k, len(counts))], 50)
        t = m.triangles[sizes >= thr]
        t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
        assert len(t) == Fx.HOLED_GRID_EXPECTED[k][1]


# ---------------------------------------------------------------- ABI rejections (no device work)
def _err():
    return _lib.lib().gsr_last_error().decode()


def _filter_count(n_tris, n_verts, k, tris=None, ws=None, ws_bytes=0):
    nv, nt = C.c_int64(-7), C.c_int64(-7)
    rc = _lib.lib().gsr_mesh_filter_count(tris, n_tris, n_verts, k, ws, ws_bytes, C.byref(nv), C.byref(nt), None)
    return rc, nv.value, nt.value


def test_filter_rejects_negative_counts():
    assert _filter_count(-1, 10, 1)[0] == GSR_E_INVALID and "n_tris" in _err()
    assert _filter_count(5, -2, 1)[0] == GSR_E_INVALID and "n_verts" in _err()
    L = _lib.lib()
    assert L.gsr_mesh_clusters(None, -1, 10, None, None, None, 0, None) == GSR_E_INVALID and "n_tris" in _err()
    assert L.gsr_mesh_clusters(None, 1, -10, None, None, None, 0, None) == GSR_E_INVALID and "n_verts" in _err()
    assert L.gsr_mesh_filter_emit(None, None, None, -3, 1, None, 0, None, None, None, None) == GSR_E_INVALID
    assert "n_tris" in _err()


def test_filter_rejects_cluster_to_keep_below_one():
    for k in (0, -1):
        assert _filter_count(5, 10, k)[0] == GSR_E_INVALID and "cluster_to_keep" in _err()


def test_filter_rejects_null_pointers_and_short_workspace():
    L = _lib.lib()
    assert _filter_count(5, 10, 1)[0] == GSR_E_INVALID and "tris" in _err()
    host = (C.c_int32 * 64)()          # never dereferenced: the checks return first
    need = L.gsr_mesh_filter_workspace_bytes(5, 10)
    assert need > 0 and L.gsr_mesh_filter_workspace_bytes(5000, 10) > need
    assert L.gsr_mesh_filter_workspace_bytes(5, 100000) > need
    rc, nv, nt = _filter_count(5, 10, 1, tris=host, ws=host, ws_bytes=need - 1)
    assert rc == GSR_E_INVALID and "ws_bytes" in _err() and (nv, nt) == (0, 0)
    assert _filter_count(5, 10, 1, tris=host, ws=None, ws_bytes=need)[0] == GSR_E_INVALID and "ws_bytes" in _err()
    need_c = L.gsr_mesh_clusters_workspace_bytes(5)
    assert 0 < need_c <= need
    assert L.gsr_mesh_clusters(host, 5, 10, host, host, host, need_c - 1, None) == GSR_E_INVALID and "ws_bytes" in _err()
    assert L.gsr_mesh_clusters(host, 5, 10, None, host, host, need_c, None) == GSR_E_INVALID and "labels" in _err()
    assert L.gsr_mesh_filter_emit(host, host, host, 5, 10, host, need - 1, host, host, host, None) == GSR_E_INVALID
    assert "ws_bytes" in _err()
    assert L.gsr_mesh_filter_emit(host, host, host, 5, 10, host, need, None, host, host, None) == GSR_E_INVALID
    assert "verts_out" in _err()


def test_filter_rejects_more_edges_than_the_sort_counts():
    L = _lib.lib()
    too_many = (2 ** 31 - 1) // 3 + 1          # 3 F > 2^31 - 1
    assert _filter_count(too_many, 10, 1)[0] == GSR_E_UNSUPPORTED and "n_tris" in _err()
    assert L.gsr_mesh_clusters(None, too_many, 10, None, None, None, 0, None) == GSR_E_UNSUPPORTED and "n_tris" in _err()
    assert _filter_count(too_many - 1, 10, 1)[0] == GSR_E_INVALID and "tris" in _err()     # the largest F passes that check
    assert _filter_count(5, 2 ** 31, 1)[0] == GSR_E_UNSUPPORTED and "n_verts" in _err()


def test_empty_mesh_launches_nothing():
    L = _lib.lib()
    rc, nv, nt = _filter_count(0, 0, 1)
    assert (rc, nv, nt) == (0, 0, 0)
    rc, nv, nt = _filter_count(0, 100, 1000)
    assert (rc, nv, nt) == (0, 0, 0)
    assert L.gsr_mesh_clusters(None, 0, 0, None, None, None, 0, None) == 0
    assert L.gsr_mesh_filter_emit(None, None, None, 0, 0, None, 0, None, None, None, None) == 0


def test_depth_aabb_rejects_bad_arguments():
    L = _lib.lib()
    f4, f16, host = (C.c_float * 4)(50, 50, 8, 8), (C.c_float * 16)(), (C.c_uint32 * 6)()
    assert L.gsr_depth_aabb(host, None, 0, 16, f4, f16, 3.0, host, None) == GSR_E_INVALID and "empty image" in _err()
    assert L.gsr_depth_aabb(None, None, 16, 16, f4, f16, 3.0, host, None) == GSR_E_INVALID and "depth" in _err()
    assert L.gsr_depth_aabb(host, None, 16, 16, f4, f16, 3.0, None, None) == GSR_E_INVALID and "bounds" in _err()
    assert L.gsr_depth_aabb(host, None, 16, 16, f4, f16, 0.0, host, None) == GSR_E_INVALID and "depth_trunc" in _err()
    f4[0] = 0.0
    assert L.gsr_depth_aabb(host, None, 16, 16, f4, f16, 3.0, host, None) == GSR_E_INVALID and "focal" in _err()


# ---------------------------------------------------------------- Python layer
def test_device_mesh_class_on_host_tensors():
    m = Fx.mixed()
    d = DeviceTriangleMesh(torch.from_numpy(m.vertices), torch.from_numpy(m.triangles), torch.from_numpy(m.vertex_colors))
    assert repr(d) == repr(m) == "TriangleMesh with 600 points and 577 triangles."
    back = d.cpu()
    assert isinstance(back, TriangleMesh)
    Fx.assert_same_mesh(back, m)
    with pytest.raises(ValueError, match="vertex_colors"):
        DeviceTriangleMesh(torch.zeros(4, 3), torch.zeros((1, 3), dtype=torch.int32), torch.zeros(3, 3))


def test_post_process_mesh_device_has_no_cpu_path():
    m = Fx.mixed()
    with pytest.raises(ValueError, match="device="):
        post_process_mesh_device(m, 1)
    d = DeviceTriangleMesh(torch.from_numpy(m.vertices), torch.from_numpy(m.triangles), torch.from_numpy(m.vertex_colors))
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        post_process_mesh_device(d, 1)
    bad = TriangleMesh(m.vertices[:10], m.triangles, m.vertex_colors[:10])
    with pytest.raises(ValueError, match="outside the vertex array"):
        post_process_mesh_device(bad, 1, device="cpu")


def test_extract_mesh_bounded_checks_the_aabb_choice():
    from gaussmart_amd.mesh import GaussianExtractor
    ex = GaussianExtractor.__new__(GaussianExtractor)
    with pytest.raises(ValueError, match="aabb must be"):
        ex.extract_mesh_bounded(aabb="numpy")
