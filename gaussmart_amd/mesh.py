"""Mesh export: the bounded TSDF path of the reference's utils/mesh_utils.py (GaussianExtractor, post_process_mesh) without
Open3D.  Fusion and marching cubes run as HIP kernels (tsdf.py); the mesh is a plain TriangleMesh of numpy arrays with a
binary PLY writer / reader that Open3D, trimesh and the reference's evaluation scripts read.

    from gaussmart_amd.mesh import GaussianExtractor, post_process_mesh
    ex = GaussianExtractor(gaussians, render, pipe, bg_color=[0, 0, 0])
    ex.reconstruction(scene.getTrainCameras())
    mesh = ex.extract_mesh_bounded(voxel_size=0.004, sdf_trunc=0.016, depth_trunc=3.0)
    post_process_mesh(mesh, cluster_to_keep=1).write_ply("fuse_post.ply")

The same on the device, from marching cubes to the PLY writer (DeviceTriangleMesh, post_process_mesh_device: the cluster
filter as kernels, no scipy):

    mesh = ex.extract_mesh_bounded(voxel_size=0.004, sdf_trunc=0.016, depth_trunc=3.0, to_host=False)
    post_process_mesh_device(mesh, cluster_to_keep=1).write_ply("fuse_post.ply")
"""
import ctypes as C
import math
import os
from functools import partial

import numpy as np
import torch

from . import _dev, _lib
from .tsdf import DepthBounds, TSDFVolume, block_aabb_of_points


class TriangleMesh:
    """vertices f32 [V,3], triangles i32 [F,3], vertex_colors f32 [V,3] in [0,1]."""

    def __init__(self, vertices=None, triangles=None, vertex_colors=None):
        self.vertices = np.zeros((0, 3), np.float32) if vertices is None else np.ascontiguousarray(vertices, np.float32)
        self.triangles = np.zeros((0, 3), np.int32) if triangles is None else np.ascontiguousarray(triangles, np.int32)
        self.vertex_colors = (np.zeros((len(self.vertices), 3), np.float32) if vertex_colors is None
                              else np.ascontiguousarray(vertex_colors, np.float32))

    def __repr__(self):
        return f"TriangleMesh with {len(self.vertices)} points and {len(self.triangles)} triangles."

    def write_ply(self, path):
        """Binary little-endian PLY: float x y z, uchar red green blue per vertex; uchar-int vertex_indices per face."""
        V, F = len(self.vertices), len(self.triangles)
        header = ("ply\nformat binary_little_endian 1.0\ncomment gaussmart_amd mesh export\n"
                  f"element vertex {V}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                  f"element face {F}\nproperty list uchar int vertex_indices\nend_header\n")
        vrec = np.empty(V, dtype=[("p", "<f4", 3), ("c", "u1", 3)])
        vrec["p"] = self.vertices
        vrec["c"] = np.round(np.clip(self.vertex_colors, 0.0, 1.0) * 255.0).astype(np.uint8)
        frec = np.empty(F, dtype=[("n", "u1"), ("i", "<i4", 3)])
        frec["n"] = 3
        frec["i"] = self.triangles
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(vrec.tobytes())
            f.write(frec.tobytes())

    @staticmethod
    def read_ply(path):
        """Reads what write_ply writes (binary little-endian, float xyz + optional uchar rgb, triangle faces)."""
        with open(path, "rb") as f:
            data = f.read()
        end = data.index(b"end_header\n") + len(b"end_header\n")
        lines = data[:end].decode("ascii").splitlines()
        if lines[0] != "ply" or "binary_little_endian" not in lines[1]:
            raise ValueError(f"{path}: not a binary little-endian PLY")
        elems, cur = [], None
        types = {"float": "<f4", "double": "<f8", "uchar": "u1", "int": "<i4", "uint": "<u4"}
        for ln in lines[2:]:
            t = ln.split()
            if t[0] == "element":
                cur = [t[1], int(t[2]), []]
                elems.append(cur)
            elif t[0] == "property":
                if t[1] == "list":
                    if t[2] != "uchar" or t[3] not in ("int", "uint"):
                        raise ValueError(f"{path}: unsupported face list {ln}")
                    cur[2].append(("list", t[4]))
                else:
                    cur[2].append((types[t[1]], t[2]))
        off, verts, cols, tris = end, None, None, None
        for name, n, props in elems:
            if name == "vertex":
                rec = np.frombuffer(data, dtype=[(p, t) for t, p in props], count=n, offset=off)
                off += rec.nbytes
                verts = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)
                if "red" in rec.dtype.names:
                    cols = np.stack([rec["red"], rec["green"], rec["blue"]], 1).astype(np.float32) / 255.0
            elif name == "face":
                rec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", 3)], count=n, offset=off)
                if n and not (rec["n"] == 3).all():
                    raise ValueError(f"{path}: only triangle faces are supported")
                off += rec.nbytes
                tris = rec["i"].astype(np.int32)
            else:
                raise ValueError(f"{path}: unexpected element {name}")
        return TriangleMesh(verts, tris, cols)


class DeviceTriangleMesh:
    """A TriangleMesh whose arrays are device tensors: vertices f32 [V,3], triangles i32 [F,3], vertex_colors f32 [V,3]."""

    def __init__(self, vertices, triangles, vertex_colors=None):
        self.vertices = vertices.to(torch.float32).reshape(-1, 3).contiguous()
        dev = self.vertices.device
        self.triangles = triangles.to(dev, torch.int32).reshape(-1, 3).contiguous()
        self.vertex_colors = (torch.zeros_like(self.vertices) if vertex_colors is None
                              else vertex_colors.to(dev, torch.float32).reshape(-1, 3).contiguous())
        if self.vertex_colors.shape != self.vertices.shape:
            raise ValueError(f"vertex_colors must be {list(self.vertices.shape)}, got {list(self.vertex_colors.shape)}")

    @property
    def device(self):
        return self.vertices.device

    def __repr__(self):
        return f"TriangleMesh with {len(self.vertices)} points and {len(self.triangles)} triangles."

    def cpu(self):
        return TriangleMesh(self.vertices.cpu().numpy(), self.triangles.cpu().numpy(), self.vertex_colors.cpu().numpy())

    def write_ply(self, path):
        self.cpu().write_ply(path)


def mesh_clusters_device(triangles, n_verts):
    """(labels, cluster_size) int32 [F] device tensors of the device int32 [F,3] triangles: the smallest triangle index of
    every triangle's edge-connected cluster and that cluster's triangle count (gsr_mesh_clusters).  Only the vertex indices
    are read, no vertex array: they must lie in [0, n_verts)."""
    L = _lib.lib()
    tris = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    if not tris.is_cuda:
        raise _lib.GsrError("mesh_clusters_device: triangles must be a device tensor (no CPU path)")
    F, dev = len(tris), tris.device
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    sizes = torch.empty(F, dtype=torch.int32, device=dev)
    ws = _dev.workspace(L.gsr_mesh_clusters_workspace_bytes(F), dev)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        _lib.check(L.gsr_mesh_clusters(C.c_void_p(tris.data_ptr()), F, int(n_verts), C.c_void_p(labels.data_ptr()),
                                       C.c_void_p(sizes.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), stream))
    return labels, sizes


def post_process_mesh_device(mesh, cluster_to_keep=1000, device=None):
    """post_process_mesh on the device (gsr_mesh_filter_*: edge sort, union-find, threshold, scans, compaction as kernels):
    the same arrays, bit for bit, as a DeviceTriangleMesh.  mesh: a DeviceTriangleMesh, or a TriangleMesh with device=."""
    print(f"post processing the mesh to have {cluster_to_keep} clusterscluster_to_kep")
    if isinstance(mesh, TriangleMesh):
        if device is None:
            raise ValueError("post_process_mesh_device: a host TriangleMesh needs device=")
        if len(mesh.triangles) and (mesh.triangles.min() < 0 or mesh.triangles.max() >= len(mesh.vertices)):
            raise ValueError("post_process_mesh_device: a triangle index lies outside the vertex array")
        mesh = DeviceTriangleMesh(torch.from_numpy(mesh.vertices).to(device), torch.from_numpy(mesh.triangles).to(device),
                                  torch.from_numpy(mesh.vertex_colors).to(device))
    if not mesh.vertices.is_cuda:
        raise _lib.GsrError("post_process_mesh_device: the mesh must live on the device (no CPU path)")
    L = _lib.lib()
    dev = mesh.device
    F, V = len(mesh.triangles), len(mesh.vertices)
    if F == 0:
        return DeviceTriangleMesh(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                                  torch.zeros((0, 3), device=dev))
    ws = _dev.workspace(L.gsr_mesh_filter_workspace_bytes(F, V), dev)
    with torch.cuda.device(dev):
        stream = _dev.stream(dev)
        nv, nt = C.c_int64(), C.c_int64()
        tp = C.c_void_p(mesh.triangles.data_ptr())
        _lib.check(L.gsr_mesh_filter_count(tp, F, V, int(cluster_to_keep), C.c_void_p(ws.data_ptr()), ws.numel(),
                                           C.byref(nv), C.byref(nt), stream))
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        cols = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        if nv.value or nt.value:
            _lib.check(L.gsr_mesh_filter_emit(C.c_void_p(mesh.vertices.data_ptr()), C.c_void_p(mesh.vertex_colors.data_ptr()), tp,
                                              F, V, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(verts.data_ptr()),
                                              C.c_void_p(cols.data_ptr()), C.c_void_p(tris.data_ptr()), stream))
    out = DeviceTriangleMesh(verts, tris, cols)
    print(f"num vertices raw {V}")
    print(f"num vertices post {len(out.vertices)}")
    return out


def post_process_mesh(mesh, cluster_to_keep=1000):
    """utils/mesh_utils.py:21-42: keep the triangle clusters (connected through shared edges) whose size is at least that of
    the cluster_to_keep-th largest one and never below 50 triangles, then drop unreferenced vertices and degenerate
    triangles.  DEVIATION: with fewer clusters than cluster_to_keep the smallest cluster sets the bar (the reference's
    np.sort(...)[-cluster_to_keep] raises IndexError there)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    print(f"post processing the mesh to have {cluster_to_keep} clusterscluster_to_kep")
    tris = mesh.triangles.astype(np.int64)
    F, V = len(tris), len(mesh.vertices)
    if F == 0:
        return TriangleMesh(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    # triangles sharing an edge: sort the 3F (edge key, triangle) pairs and link neighbours with equal keys
    e = np.sort(np.stack([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]], 1).reshape(-1, 2), axis=1)
    key = e[:, 0] * V + e[:, 1]
    order = np.argsort(key, kind="stable")
    ks, tid = key[order], order // 3
    same = ks[1:] == ks[:-1]
    g = coo_matrix((np.ones(int(same.sum())), (tid[:-1][same], tid[1:][same])), shape=(F, F))
    _, labels = connected_components(g, directed=False)
    counts = np.bincount(labels)
    k = min(int(cluster_to_keep), len(counts))
    n_cluster = max(np.sort(counts)[-k], 50)
    keep = counts[labels] >= n_cluster
    kept = tris[keep]
    used = np.zeros(V, bool)
    used[kept.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    kept = remap[kept]
    kept = kept[(kept[:, 0] != kept[:, 1]) & (kept[:, 1] != kept[:, 2]) & (kept[:, 0] != kept[:, 2])]
    out = TriangleMesh(mesh.vertices[used], kept, mesh.vertex_colors[used])
    print(f"num vertices raw {V}")
    print(f"num vertices post {len(out.vertices)}")
    return out


def focus_point_fn(poses):
    """utils/render_utils.py:68-74: nearest point to all focal axes of camera-to-world poses [N,3,4]."""
    directions, origins = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - directions * np.transpose(directions, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ origins).mean(0)[:, 0]


def camera_intrinsics(cam):
    """to_cam_open3d (utils/mesh_utils.py:44-70): fx = W / (2 tan(FoVx / 2)), cx = (W - 1) / 2, the same for y."""
    W, H = cam.image_width, cam.image_height
    return (W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2)), (W - 1) / 2, (H - 1) / 2)


def _save_img_u8(img, path):
    from PIL import Image
    Image.fromarray((np.clip(np.nan_to_num(img), 0.0, 1.0) * 255.0).astype(np.uint8)).save(path, "PNG")


def _save_img_f32(depth, path):
    from PIL import Image
    Image.fromarray(np.nan_to_num(depth).astype(np.float32)).save(path, "TIFF")


class GaussianExtractor:
    """utils/mesh_utils.py:73-171, 272-295 (bounded path).  The rendered maps stay on the device."""

    def __init__(self, gaussians, render, pipe, bg_color=None):
        if bg_color is None:
            bg_color = [0, 0, 0]
        device = gaussians.get_xyz.device
        background = torch.tensor(bg_color, dtype=torch.float32, device=device)
        self.gaussians = gaussians
        self.render = partial(render, pipe=pipe, bg_color=background)
        self.clean()

    @torch.no_grad()
    def clean(self):
        self.depthmaps = []
        self.rgbmaps = []
        self.viewpoint_stack = []

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack):
        self.clean()
        self.viewpoint_stack = viewpoint_stack
        for cam in self.viewpoint_stack:
            pkg = self.render(cam, self.gaussians)
            self.rgbmaps.append(pkg["render"])
            self.depthmaps.append(pkg["surf_depth"])
        self.estimate_bounding_sphere()

    def estimate_bounding_sphere(self):
        c2ws = np.array([np.linalg.inv(cam.world_view_transform.T.cpu().numpy().astype(np.float64))
                         for cam in self.viewpoint_stack])
        poses = c2ws[:, :3, :] @ np.diag([1, -1, -1, 1])
        center = focus_point_fn(poses)
        self.radius = float(np.linalg.norm(c2ws[:, :3, 3] - center, axis=-1).min())
        self.center = torch.from_numpy(center).float()
        print(f"The estimated bounding radius is {self.radius:.2f}")
        print(f"Use at least {2.0 * self.radius:.2f} for depth_trunc")

    def _masked_depth(self, i, mask_backgrond):
        depth = self.depthmaps[i].float()
        mask = getattr(self.viewpoint_stack[i], "gt_alpha_mask", None)
        if mask_backgrond and mask is not None:
            depth = torch.where(mask.to(depth.device).reshape(depth.shape) < 0.5, torch.zeros_like(depth), depth)
        return depth

    @torch.no_grad()
    def block_aabb(self, voxel_size, sdf_trunc, depth_trunc, mask_backgrond=True):
        """Block AABB of the back-projected valid depth of every view, padded by sdf_trunc (tsdf.block_aabb_of_points)."""
        lo = np.full(3, np.inf)
        hi = np.full(3, -np.inf)
        for i, cam in enumerate(self.viewpoint_stack):
            d = self._masked_depth(i, mask_backgrond)[0]
            fx, fy, cx, cy = camera_intrinsics(cam)
            H, W = d.shape
            v, u = torch.meshgrid(torch.arange(H, device=d.device, dtype=torch.float32),
                                  torch.arange(W, device=d.device, dtype=torch.float32), indexing="ij")
            ok = (d > 0) & (d <= depth_trunc)
            if not bool(ok.any()):
                continue
            z = d[ok]
            pc = torch.stack([(u[ok] - cx) * z / fx, (v[ok] - cy) * z / fy, z], 1)
            c2w = torch.linalg.inv(cam.world_view_transform.T.double()).float().to(d.device)
            pw = pc @ c2w[:3, :3].T + c2w[:3, 3]
            lo = np.minimum(lo, pw.min(0).values.cpu().numpy())
            hi = np.maximum(hi, pw.max(0).values.cpu().numpy())
        if not np.isfinite(lo).all():
            return [0, 0, 0], [0, 0, 0]
        return block_aabb_of_points(lo, hi, voxel_size, sdf_trunc)

    @torch.no_grad()
    def block_aabb_device(self, voxel_size, sdf_trunc, depth_trunc, mask_backgrond=True):
        """block_aabb through gsr_depth_aabb: one kernel per view on a running device AABB, ONE host read after the last
        view (and one for all the camera matrices before the first)."""
        if not self.viewpoint_stack:
            return [0, 0, 0], [0, 0, 0]
        dev = self.depthmaps[0].device
        w2cs = torch.stack([cam.world_view_transform.T for cam in self.viewpoint_stack]).cpu().double()
        c2ws = torch.linalg.inv(w2cs).float().numpy()
        bounds = DepthBounds(dev)
        for i, cam in enumerate(self.viewpoint_stack):
            bounds.add(self._masked_depth(i, mask_backgrond), camera_intrinsics(cam), c2ws[i], depth_trunc)
        ext = bounds.read()
        if ext is None:
            return [0, 0, 0], [0, 0, 0]
        return block_aabb_of_points(ext[0], ext[1], voxel_size, sdf_trunc)

    @torch.no_grad()
    def extract_mesh_bounded(self, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3, mask_backgrond=True, aabb="device",
                             to_host=True):
        """aabb: "device" (block_aabb_device) or "torch" (block_aabb) -- the AABB only places the grid, the mesh does not
        depend on which pass found it; to_host=False: a DeviceTriangleMesh."""
        if aabb not in ("device", "torch"):
            raise ValueError(f"aabb must be 'device' or 'torch', got {aabb!r}")
        print("Running tsdf volume integration ...")
        print(f"voxel_size: {voxel_size}")
        print(f"sdf_trunc: {sdf_trunc}")
        print(f"depth_truc: {depth_trunc}")
        aabb = (self.block_aabb_device if aabb == "device" else self.block_aabb)(voxel_size, sdf_trunc, depth_trunc,
                                                                                mask_backgrond)
        volume = TSDFVolume(voxel_size, sdf_trunc, aabb, device=self.gaussians.get_xyz.device)
        for i, cam in enumerate(self.viewpoint_stack):
            volume.integrate(self._masked_depth(i, mask_backgrond), self.rgbmaps[i], camera_intrinsics(cam),
                             cam.world_view_transform.T, depth_trunc)
        return volume.extract_triangle_mesh(to_host=to_host)

    def extract_mesh_unbounded(self, resolution=1024):
        raise NotImplementedError(
            "extract_mesh_unbounded (utils/mesh_utils.py:173-270: contracted-space grid with bilinear sampling) is not "
            "implemented yet; it is the follow-up of the bounded mesh export.  Use extract_mesh_bounded.")

    @torch.no_grad()
    def export_image(self, path, host=False):
        """renders/NNNNN.png, gt/NNNNN.png and vis/depth_NNNNN.tiff of every view.  Default: the colours become u8 and the
        depth is cleaned on the device (gaussmart_amd/frames.py) and only those bytes are copied down; host=True copies the
        fp32 maps and converts with numpy.  Both write the same files, byte for byte."""
        render_path, gts_path, vis_path = (os.path.join(path, d) for d in ("renders", "gt", "vis"))
        for d in (render_path, vis_path, gts_path):
            os.makedirs(d, exist_ok=True)
        if not host:
            from PIL import Image
            from .frames import clean_depth, to_u8
            for idx, cam in enumerate(self.viewpoint_stack):
                dev = self.rgbmaps[idx].device
                if cam.original_image is not None:
                    Image.fromarray(to_u8(cam.original_image[0:3].to(dev)).cpu().numpy()).save(
                        os.path.join(gts_path, f"{idx:05d}.png"), "PNG")
                Image.fromarray(to_u8(self.rgbmaps[idx]).cpu().numpy()).save(os.path.join(render_path, f"{idx:05d}.png"), "PNG")
                Image.fromarray(clean_depth(self.depthmaps[idx][0]).cpu().numpy()).save(
                    os.path.join(vis_path, f"depth_{idx:05d}.tiff"), "TIFF")
            return
        for idx, cam in enumerate(self.viewpoint_stack):
            if cam.original_image is not None:
                _save_img_u8(cam.original_image[0:3].permute(1, 2, 0).cpu().numpy(), os.path.join(gts_path, f"{idx:05d}.png"))
            _save_img_u8(self.rgbmaps[idx].permute(1, 2, 0).cpu().numpy(), os.path.join(render_path, f"{idx:05d}.png"))
            _save_img_f32(self.depthmaps[idx][0].cpu().numpy(), os.path.join(vis_path, f"depth_{idx:05d}.tiff"))
