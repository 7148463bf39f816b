"""Block-sparse TSDF volume on the HIP library (include/gsr.h, "mesh export"): what the reference gets from Open3D's
ScalableTSDFVolume with RGB8 colour (utils/mesh_utils.py:142-167), fusion and marching cubes both as kernels.

    vol = TSDFVolume(voxel_size, sdf_trunc, block_aabb)
    vol.integrate(depth[1,H,W], rgb[3,H,W], (fx, fy, cx, cy), w2c[4,4], depth_trunc, mask=None)   # per view
    mesh = vol.extract_triangle_mesh()                                                            # mesh.TriangleMesh
    mesh = vol.extract_triangle_mesh(to_host=False)                                               # mesh.DeviceTriangleMesh

block_aabb = (lo, hi): integer block coordinates, hi exclusive; block b holds voxels [16 b, 16 b + 16) and voxel g has its
centre at (g + 0.5) * voxel_size.  block_aabb_of_points() derives one from the extent of the back-projected depth.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _dev, _lib

BLOCK = 16


def block_aabb_of_points(pmin, pmax, voxel_size, sdf_trunc):
    """Block AABB that holds every block a depth sample in [pmin, pmax] can touch (its [p - sdf_trunc, p + sdf_trunc]
    box), with one block of slack against float rounding of the kernel's own floor decisions."""
    bl = BLOCK * float(voxel_size)
    lo = [int(math.floor((float(pmin[a]) - sdf_trunc) / bl)) - 1 for a in range(3)]
    hi = [int(math.floor((float(pmax[a]) + sdf_trunc) / bl)) + 2 for a in range(3)]
    return lo, hi


def _host_floats(values, n, name):
    arr = np.asarray(values.detach().cpu() if torch.is_tensor(values) else values, dtype=np.float64).reshape(-1)
    if arr.size != n:
        raise ValueError(f"{name} needs {n} values, got {arr.size}")
    return (C.c_float * n)(*arr.tolist())


def _intrinsics(intrinsics):
    """(fx, fy, cx, cy) or a 3x3 K."""
    arr = np.asarray(intrinsics.detach().cpu() if torch.is_tensor(intrinsics) else intrinsics, dtype=np.float64)
    if arr.shape == (3, 3):
        arr = np.array([arr[0, 0], arr[1, 1], arr[0, 2], arr[1, 2]])
    return _host_floats(arr, 4, "intrinsics")


class TSDFVolume:
    def __init__(self, voxel_size, sdf_trunc, block_aabb, device=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        lo, hi = (tuple(int(v) for v in b) for b in block_aabb)
        self.voxel_size, self.sdf_trunc = float(voxel_size), float(sdf_trunc)
        v = _lib.GsrTsdfVolume()
        v.voxel_size, v.sdf_trunc = self.voxel_size, self.sdf_trunc
        v.block_lo[:], v.block_hi[:] = lo, hi
        n_blocks, ws_bytes, slot_block_off = C.c_int64(), C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().gsr_tsdf_sizes(C.byref(v), C.byref(n_blocks), C.byref(ws_bytes), C.byref(slot_block_off)))
        self._slot_block_offset = slot_block_off.value
        self.block_lo, self.block_hi, self.n_blocks = lo, hi, n_blocks.value
        self.block_index = torch.full((max(1, self.n_blocks),), -1, dtype=torch.int32, device=self.device)
        self.workspace = torch.zeros(max(1, ws_bytes.value), dtype=torch.uint8, device=self.device)
        self.pool = torch.zeros((5, 0, BLOCK ** 3), dtype=torch.float32, device=self.device)
        v.block_index, v.workspace, v.workspace_bytes = self.block_index.data_ptr(), self.workspace.data_ptr(), ws_bytes.value
        v.pool, v.pool_blocks = None, 0
        self._v = v

    @property
    def n_alloc(self):
        return int(self._v.n_alloc)

    def _grow_pool(self, need):
        cap = self.pool.shape[1]
        if need <= cap:
            return
        new = torch.zeros((5, max(need, cap + cap // 2, 64), BLOCK ** 3), dtype=torch.float32, device=self.device)
        if cap:
            new[:, :cap].copy_(self.pool)
        self.pool = new
        self._v.pool, self._v.pool_blocks = new.data_ptr(), new.shape[1]

    def integrate(self, depth, rgb, intrinsics, w2c, depth_trunc, mask=None):
        """Fuse one view.  depth [1,H,W] (or [H,W]), rgb [3,H,W] in [0,1], intrinsics (fx, fy, cx, cy) or K, w2c [4,4]
        world-to-camera (p_cam = w2c p_world), mask [1,H,W] / [H,W] (False: pixel ignored) or None.  Raises if a depth
        sample touches a block outside the AABB."""
        L = _lib.lib()
        d = depth.detach().to(self.device, torch.float32).contiguous()
        if d.dim() == 3:
            d = d[0]
        H, W = (d.shape[0], d.shape[1]) if d.dim() == 2 else (0, 0)
        c = rgb.detach().to(self.device, torch.float32).contiguous()
        if c.shape != (3, H, W):
            raise ValueError(f"rgb must be [3,{H},{W}], got {list(c.shape)}")
        m = None
        if mask is not None:
            m = mask.detach().to(self.device).reshape(H, W).to(torch.uint8).contiguous()
        intr, M = _intrinsics(intrinsics), _host_floats(w2c, 16, "w2c")
        if self.n_blocks == 0 and bool(((d > 0) & (d <= depth_trunc) & (m.bool() if m is not None else True)).any()):
            raise _lib.GsrError("the TSDF block AABB is empty but the view has valid depth")
        mp = C.c_void_p(m.data_ptr()) if m is not None else None
        with torch.cuda.device(self.device):
            stream = _dev.stream(self.device)
            n_touched = C.c_int64()
            _lib.check(L.gsr_tsdf_touch(C.byref(self._v), C.c_void_p(d.data_ptr()), mp, H, W, intr, M, float(depth_trunc),
                                        C.byref(n_touched), stream))
            self._grow_pool(self.n_alloc)
            _lib.check(L.gsr_tsdf_integrate(C.byref(self._v), C.c_void_p(d.data_ptr()), mp, C.c_void_p(c.data_ptr()), H, W,
                                            intr, M, float(depth_trunc), n_touched.value, stream))
        return n_touched.value

    @classmethod
    def from_dense(cls, voxel_size, sdf_trunc, tsdf, weight, colour=None, device=None, block_lo=(0, 0, 0), blocks=None,
                   slot_order=None):
        """A volume holding a dense field [X,Y,Z] whose voxel (0, 0, 0) is grid voxel 16 * block_lo (the block AABB is
        block_lo + [0, ceil(X/16)) x ...); colour [X,Y,Z,3] on the 0..255 scale.  Voxels beyond the field keep weight 0.
        blocks: bool [ceil(X/16), ceil(Y/16), ceil(Z/16)], the blocks to allocate (None: all); the others stay unallocated.
        slot_order: a permutation of the allocated blocks' grid-order ranks, slot s holding the block of rank
        slot_order[s] (None: slots in grid order).  A test and loading aid: fusion never builds a volume this way."""
        tsdf = torch.as_tensor(tsdf, dtype=torch.float32)
        X, Y, Z = tsdf.shape
        dims = [-(-s // BLOCK) for s in (X, Y, Z)]
        lo = [int(v) for v in block_lo]
        vol = cls(voxel_size, sdf_trunc, (lo, [l + d for l, d in zip(lo, dims)]), device=device)
        pad = torch.zeros((5, dims[0] * BLOCK, dims[1] * BLOCK, dims[2] * BLOCK), dtype=torch.float32)
        pad[0, :X, :Y, :Z] = tsdf
        pad[1, :X, :Y, :Z] = torch.as_tensor(weight, dtype=torch.float32)
        if colour is not None:
            pad[2:5, :X, :Y, :Z] = torch.as_tensor(colour, dtype=torch.float32).permute(3, 0, 1, 2)
        # [5, bx, 16, by, 16, bz, 16] -> [5, bz, by, bx, z, y, x] -> [5, linear block id, 4096]
        pad = pad.reshape(5, dims[0], BLOCK, dims[1], BLOCK, dims[2], BLOCK).permute(0, 5, 3, 1, 6, 4, 2)
        pad = pad.reshape(5, vol.n_blocks, BLOCK ** 3)
        if blocks is None:
            ids = torch.arange(vol.n_blocks, dtype=torch.int64)
        else:
            sel = torch.as_tensor(np.asarray(blocks, dtype=bool))
            if tuple(sel.shape) != tuple(dims):
                raise ValueError(f"blocks must be {dims}, got {list(sel.shape)}")
            ids = torch.nonzero(sel.permute(2, 1, 0).reshape(-1)).flatten()   # linear ids (x fastest), grid order
        n = len(ids)
        if slot_order is not None:
            order = torch.as_tensor(np.asarray(slot_order, dtype=np.int64))
            if not torch.equal(torch.sort(order).values, torch.arange(n)):
                raise ValueError(f"slot_order must be a permutation of range({n})")
            ids = ids[order]
        vol._grow_pool(n)
        vol.pool[:, :n] = pad[:, ids].to(vol.device)
        ids = ids.to(torch.int32).to(vol.device)
        vol.block_index[ids.long()] = torch.arange(n, dtype=torch.int32, device=vol.device)
        vol._slot_block()[:n] = ids
        vol._v.n_alloc = n
        return vol

    def voxels(self):
        """(grid voxel coordinates int64 [n_alloc * 4096, 3], tsdf, weight, colour [.., 3] on the 0..255 scale) of every
        allocated voxel, slot order (test and debugging aid)."""
        A = self.n_alloc
        ws_slot_block = self._slot_block()[:A].long()
        dim = [h - l for l, h in zip(self.block_lo, self.block_hi)]
        bx, by, bz = ws_slot_block % dim[0], (ws_slot_block // dim[0]) % dim[1], ws_slot_block // (dim[0] * dim[1])
        blk = torch.stack([bx, by, bz], 1) + torch.tensor(self.block_lo, device=self.device)
        l = torch.arange(BLOCK ** 3, device=self.device)
        loc = torch.stack([l % BLOCK, (l // BLOCK) % BLOCK, l // (BLOCK * BLOCK)], 1)
        g = (blk[:, None, :] * BLOCK + loc[None]).reshape(-1, 3)
        p = self.pool[:, :A].reshape(5, -1)
        return g, p[0], p[1], p[2:5].T

    def _slot_block(self):
        # the slot -> block map inside the workspace, where gsr_tsdf_sizes says it is
        off, n = self._slot_block_offset, self.n_blocks
        return self.workspace[off:off + 4 * n].view(torch.int32)

    def extract_triangle_mesh(self, to_host=True):
        """Marching cubes over the allocated blocks: a mesh.TriangleMesh (numpy), or with to_host=False a
        mesh.DeviceTriangleMesh whose arrays stay on the device (no copy)."""
        from .mesh import DeviceTriangleMesh, TriangleMesh
        L = _lib.lib()
        A = self.n_alloc
        ws = _dev.workspace(L.gsr_mcubes_workspace_bytes(A), self.device)
        with torch.cuda.device(self.device):
            stream = _dev.stream(self.device)
            nv, nt = C.c_int64(), C.c_int64()
            _lib.check(L.gsr_mcubes_count(C.byref(self._v), C.c_void_p(ws.data_ptr()), ws.numel(), C.byref(nv), C.byref(nt),
                                          stream))
            verts = torch.empty((nv.value, 3), dtype=torch.float32, device=self.device)
            cols = torch.empty((nv.value, 3), dtype=torch.float32, device=self.device)
            tris = torch.empty((nt.value, 3), dtype=torch.int32, device=self.device)
            if nv.value or nt.value:
                _lib.check(L.gsr_mcubes_emit(C.byref(self._v), C.c_void_p(ws.data_ptr()), ws.numel(),
                                             C.c_void_p(verts.data_ptr()), C.c_void_p(cols.data_ptr()),
                                             C.c_void_p(tris.data_ptr()), stream))
        if not to_host:
            return DeviceTriangleMesh(verts, tris, cols)
        return TriangleMesh(verts.cpu().numpy(), tris.cpu().numpy(), cols.cpu().numpy())


class DepthBounds:
    """Running world-space AABB of back-projected valid depth on the device (gsr_depth_aabb): add() enqueues one kernel per
    view and reads nothing back; read() is the one host read, after the last view."""

    def __init__(self, device):
        self.device = torch.device(device)
        # order-preserving u32 keys of floats: (max, max, max, 0, 0, 0) = nothing seen yet
        self.words = torch.tensor([-1, -1, -1, 0, 0, 0], dtype=torch.int32, device=self.device)

    def add(self, depth, intrinsics, c2w, depth_trunc, mask=None):
        """depth [1,H,W] / [H,W], intrinsics (fx, fy, cx, cy) or K, c2w [4,4] camera-to-world, mask [H,W] (False: pixel
        ignored) or None; the tensors must stay alive until the stream has run the kernel (read() waits for it)."""
        d = depth.detach().to(self.device, torch.float32).contiguous()
        if d.dim() == 3:
            d = d[0]
        H, W = d.shape
        m = None
        if mask is not None:
            m = mask.detach().to(self.device).reshape(H, W).to(torch.uint8).contiguous()
        intr, M = _intrinsics(intrinsics), _host_floats(c2w, 16, "c2w")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            _lib.check(_lib.lib().gsr_depth_aabb(C.c_void_p(d.data_ptr()), C.c_void_p(m.data_ptr()) if m is not None else None,
                                                 H, W, intr, M, float(depth_trunc), C.c_void_p(self.words.data_ptr()),
                                                 C.c_void_p(stream.cuda_stream)))
            d.record_stream(stream)
            if m is not None:
                m.record_stream(stream)

    def read(self):
        """(lo, hi) float32 [3] each, or None when no pixel was valid."""
        k = self.words.cpu().numpy().view(np.uint32)
        if (k[:3] == 0xFFFFFFFF).all() and (k[3:] == 0).all():
            return None
        bits = np.where(k & 0x80000000, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
        f = bits.view(np.float32)
        return f[:3].copy(), f[3:].copy()
