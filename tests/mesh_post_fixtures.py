"""Meshes for the cluster-filter tests (tests/test_mesh_post_cpu.py, tests/test_gpu_mesh_post.py), built from fixed seeds,
and the host references: gaussmart_amd.mesh.post_process_mesh for the filter, scipy's connected_components for the labels."""
import contextlib
import functools
import io

import numpy as np

from gaussmart_amd.mesh import TriangleMesh, post_process_mesh

# vertices / triangles the host post_process_mesh keeps, per cluster_to_keep (checked in tests/test_mesh_post_cpu.py)
MIXED_EXPECTED = {1: (502, 501), 2: (567, 564), 3: (567, 564), 50: (567, 564)}
HOLED_GRID_EXPECTED = {1: (600, 749), 3: (1337, 1632), 10: (2693, 3258), 1000: (5536, 6660)}
HOLED_GRID_TRIANGLES = 11953
KEEP = (1, 2, 3, 10, 50, 1000)


def strip(n_tris, offset):
    """The triangles of a strip of n_tris triangles (edge-connected), vertex indices from offset."""
    return np.array([[i, i + 1, i + 2] for i in range(n_tris)], dtype=np.int64) + offset


def _mesh(n_verts, tris, seed):
    rng = np.random.default_rng(seed)
    verts = rng.random((n_verts, 3)).astype(np.float32)
    cols = rng.random((n_verts, 3)).astype(np.float32)
    return TriangleMesh(verts, np.asarray(tris, dtype=np.int32), cols)


@functools.lru_cache(maxsize=None)
def mixed(big_strips=True):
    """(A): strips of 10, 60 and 500 triangles, a non-manifold edge (12, 13) shared by five triangles (one of the extra three
    with reversed winding), two degenerate triangles, a duplicate, an isolated triangle and unused vertices; 600 vertices,
    triangle ids permuted.  big_strips=False: without the 60 and 500 strips (every cluster below 50)."""
    parts = [strip(10, 0)]
    if big_strips:
        parts += [strip(60, 12), strip(500, 74)]
    parts.append(np.array([[12, 13, 580], [13, 12, 581], [12, 13, 582],      # on edge (12, 13); the second is reversed
                           [100, 100, 101], [200, 201, 200],                 # degenerate
                           [80, 81, 82],                                     # duplicate of a strip triangle
                           [590, 591, 592]]))                                # isolated
    tris = np.concatenate(parts)
    tris = tris[np.random.default_rng(0).permutation(len(tris))]
    return _mesh(600, tris, 1)


@functools.lru_cache(maxsize=None)
def holed_grid():
    """(B): the 2 * 96^2 triangles of a 97 x 97 vertex grid, each dropped with probability 0.35, the rest permuted."""
    n = 97
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    tris = np.concatenate([np.stack([a, a + 1, a + n], 1), np.stack([a + 1, a + n + 1, a + n], 1)])
    rng = np.random.default_rng(7)
    tris = tris[rng.random(len(tris)) > 0.35]
    tris = tris[rng.permutation(len(tris))]
    return _mesh(n * n, tris, 2)


@functools.lru_cache(maxsize=None)
def snake(n_tris=200_000):
    """(C): one strip of n_tris triangles, ids permuted."""
    tris = strip(n_tris, 0)
    tris = tris[np.random.default_rng(11).permutation(n_tris)]
    return _mesh(n_tris + 2, tris, 3)


def reference_labels(tris, n_verts):
    """Per triangle: the smallest triangle index of its edge-connected component and the component's size (scipy)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(tris, dtype=np.int64)
    F = len(t)
    e = np.sort(np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 1).reshape(-1, 2), axis=1)
    order = np.lexsort((e[:, 1], e[:, 0]))
    es, tid = e[order], order // 3
    same = (es[1:] == es[:-1]).all(1)
    g = coo_matrix((np.ones(int(same.sum())), (tid[:-1][same], tid[1:][same])), shape=(F, F))
    _, comp = connected_components(g, directed=False)
    first = np.full(comp.max() + 1, F, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(F))
    return first[comp].astype(np.int32), np.bincount(comp)[comp].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _host_filtered(name, arg, k):
    mesh = {"mixed": mixed, "holed_grid": holed_grid, "snake": snake}[name](*arg)
    with contextlib.redirect_stdout(io.StringIO()):
        return post_process_mesh(mesh, k)


def host_filtered(name, k, *arg):
    """post_process_mesh(fixture, k) on the host, computed once per (fixture, k) and shared: do not modify."""
    return _host_filtered(name, arg, k)


def assert_same_mesh(got, want):
    """np.array_equal on all three arrays, dtypes and shapes included."""
    for a in ("vertices", "triangles", "vertex_colors"):
        g, w = getattr(got, a), getattr(want, a)
        assert g.dtype == w.dtype and g.shape == w.shape, (a, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), a
