"""Projective TSDF fusion of range images on the device (csrc/tsdf.hip, include/lidarnerf_hip.h lnh_tsdf_* and lnh_mesh_*): the
meshing function of the mesh baseline's fit.  LidarNVSMeshing (lidarnvs/lidarnvs_meshing.py) is a base class whose children
plug in a `meshing_func`; the reference's child runs Open3D's Poisson reconstruction on a cloud with estimated normals.  A
training sequence here is a set of range images with poses, which is exactly what TSDF fusion takes: no normals, no solver, and
the free space every ray proves empty is used.  Every stage is a pure function of its inputs.

Nearest-pixel depth, unit weights, the column wrap, the fill of unobserved points and the trim of the mesh to observed lattice
points are this package's own choices; nothing here is pinned against Open3D.  No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _hip
from ._cellgrid import device as _device

_SYMBOLS = ("lnh_tsdf_integrate", "lnh_tsdf_finalize", "lnh_mesh_vertex_observed", "lnh_mesh_filter_workspace_size",
            "lnh_mesh_filter_count", "lnh_mesh_filter_emit")


def _f3(values):
    return (C.c_float * 3)(*[float(v) for v in values])


def vertex_observed(vertices, count, min_count=1):
    """keep u8 [V] of marching-cubes vertices [V,3] (index units) over the lattice's count [nx,ny,nz]: 1 iff both lattice ends of
    the vertex's edge were observed (lnh_mesh_vertex_observed)."""
    _hip.require_symbols(_SYMBOLS, "TSDF fusion")
    _hip.require_cuda(vertices, count)
    V = int(vertices.shape[0])
    keep = torch.empty(V, dtype=torch.uint8, device=vertices.device)
    if V:
        nx, ny, nz = count.shape
        with torch.cuda.device(vertices.device):
            _hip.call("lnh_mesh_vertex_observed", vertices.data_ptr(), V, count.data_ptr(), nx, ny, nz, int(min_count),
                      keep.data_ptr())
    return keep


def filter_mesh(vertices, triangles, keep):
    """Open3D's remove_vertices_by_mask with keep = 1 meaning "stays" (lnh_mesh_filter_*): the kept vertices in order, the
    triangles whose three corners are kept in order, renumbered.  One host read of the two counts between count and emit."""
    _hip.require_symbols(_SYMBOLS, "TSDF fusion")
    _hip.require_cuda(vertices, triangles, keep)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("lidarnerf.tsdf.filter_mesh: not while a stream is capturing (it reads counts back)")
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    dev = vertices.device
    if keep.dtype != torch.uint8 or keep.numel() != V or triangles.dtype != torch.int32 or vertices.dtype != torch.float32:
        raise ValueError("filter_mesh: vertices f32 [V,3], triangles i32 [T,3], keep u8 [V]")
    if V == 0 or T == 0:
        return vertices[:0].clone(), triangles[:0].clone()
    with torch.cuda.device(dev):
        need = int(_hip.lib().lnh_mesh_filter_workspace_size(V, T))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        counts = torch.empty(4, dtype=torch.int32, device=dev)
        _hip.call("lnh_mesh_filter_count", keep.data_ptr(), V, triangles.data_ptr(), T, ws.data_ptr(), ws.numel(), counts.data_ptr())
        Vk, Tk = (c & 0xffffffff for c in counts.tolist()[:2])  # the one host read
        out_v = torch.empty((Vk, 3), dtype=torch.float32, device=dev)
        out_t = torch.empty((Tk, 3), dtype=torch.int32, device=dev)
        if Vk:
            _hip.call("lnh_mesh_filter_emit", vertices.data_ptr(), keep.data_ptr(), V, triangles.data_ptr(), T, ws.data_ptr(),
                      ws.numel(), out_v.data_ptr(), Vk, _hip.ptr(out_t) if Tk else None, Tk)
    return out_v, out_t


class TSDFVolume:
    """A truncated signed-distance volume averaged over range images.  box: (min[3], max[3]) in world units.  The lattice has
    `resolution` points per axis from end to end of the box, or — with voxel_size — points voxel_size apart starting at the box's
    minimum, ceil(extent / voxel_size) per axis (at least 2), so the numbers of points differ from axis to axis.
    truncation: None = 3 x the largest step."""

    def __init__(self, box, resolution=256, voxel_size=None, truncation=None, device=None):
        _hip.require_symbols(_SYMBOLS, "TSDF fusion")
        lo, hi = (np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64).reshape(3) for b in box)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            raise ValueError(f"TSDFVolume: box must be finite with max > min on every axis, got {lo.tolist()} .. {hi.tolist()}")
        if voxel_size is None:
            if int(resolution) < 2:
                raise ValueError("TSDFVolume: resolution must be at least 2")
            self.dims = (int(resolution),) * 3
            step = (hi - lo) / (int(resolution) - 1)
        else:
            if not (float(voxel_size) > 0 and math.isfinite(float(voxel_size))):
                raise ValueError("TSDFVolume: voxel_size must be positive and finite")
            self.dims = tuple(max(2, int(math.ceil(e / float(voxel_size) - 1e-6))) for e in (hi - lo))
            step = np.full(3, float(voxel_size))
        if self.dims[0] * self.dims[1] * self.dims[2] >= 1 << 31:
            raise ValueError(f"TSDFVolume: a lattice of {self.dims} points does not fit 31-bit indices")
        self.lo, self.step = lo.astype(np.float32), step.astype(np.float32)
        self.truncation = float(np.float32(3.0) * self.step.max()) if truncation is None else float(np.float32(truncation))
        if not (self.truncation > 0 and math.isfinite(self.truncation)):
            raise ValueError("TSDFVolume: truncation must be positive and finite")
        self.device = _device() if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume: the volume lives on the GPU (no CPU fallback)")
        self.sum = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.count = torch.zeros(self.dims, dtype=torch.int32, device=self.device)  # (read as u32 by the kernels)
        self.frames = 0

    def integrate(self, panos, poses, lidar_K, max_depth=80):
        """Add F frames: panos [F,H,W] (or [H,W]) depths, a value <= 0 or not finite meaning no observation; poses [F,4,4] (or
        [4,4]) lidar -> world, inverted with nvs.inverse_pose on the device; lidar_K = (fov_up, fov) in degrees.  Any number of
        calls; the frames of one call are taken in order.  Returns self."""
        from .nvs import inverse_pose
        to_t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a  # (a copy: read-only arrays)
        panos, poses = to_t(panos), to_t(poses)
        if not torch.is_tensor(panos) or not torch.is_tensor(poses):
            raise TypeError("TSDFVolume.integrate: panos and poses must be tensors or NumPy arrays")
        panos = panos.detach().to(self.device, torch.float32)
        poses = poses.detach().to(self.device, torch.float32)
        if panos.dim() == 2:
            panos = panos[None]
        if poses.dim() == 2:
            poses = poses[None]
        if panos.dim() != 3 or poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] != panos.shape[0]:
            raise ValueError(f"TSDFVolume.integrate: panos [F,H,W] and poses [F,4,4], got {tuple(panos.shape)} and "
                             f"{tuple(poses.shape)}")
        K = [float(x) for x in (lidar_K.tolist() if hasattr(lidar_K, "tolist") else lidar_K)]
        if len(K) != 2:
            raise ValueError("TSDFVolume.integrate: lidar_K must be (fov_up, fov)")
        F, H, W = (int(n) for n in panos.shape)
        panos = panos.contiguous()
        w2l = torch.stack([inverse_pose(p)[:3].reshape(12) for p in poses]).contiguous() if F else poses.reshape(0, 12)
        nx, ny, nz = self.dims
        with torch.cuda.device(self.device):
            _hip.call("lnh_tsdf_integrate", panos.data_ptr(), w2l.data_ptr(), F, H, W, K[0], K[1], float(max_depth), _f3(self.lo),
                      _f3(self.step), nx, ny, nz, self.truncation, self.sum.data_ptr(), self.count.data_ptr())
        self.frames += F
        return self

    def volume(self, min_count=1):
        """fp32 [nx,ny,nz]: -(sum / count) where count >= min_count (free space negative, matter positive), +1 elsewhere."""
        nx, ny, nz = self.dims
        vol = torch.empty(self.dims, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.call("lnh_tsdf_finalize", self.sum.data_ptr(), self.count.data_ptr(), nx, ny, nz, int(min_count), vol.data_ptr())
        return vol

    def to_world(self, vertices):
        """Index units -> world units: lo + v * step in float64 on the lattice's float32 numbers, rounded to float32 once."""
        lo = torch.from_numpy(self.lo.astype(np.float64)).to(vertices.device)
        step = torch.from_numpy(self.step.astype(np.float64)).to(vertices.device)
        return (lo[None, :] + vertices.double() * step[None, :]).float()

    def extract_mesh(self, min_count=1):
        """(vertices fp32 [V,3] in world units, triangles int32 [T,3]) on the device: volume(min_count), marching cubes at 0
        (nerf.mesh.marching_cubes), the vertices that rest on observed lattice points (vertex_observed), filter_mesh, to_world.
        Normals face the sensors.  Raises on an empty result."""
        from .nerf.mesh import marching_cubes
        vertices, triangles = marching_cubes(self.volume(min_count), 0.0)
        keep = vertex_observed(vertices, self.count, min_count)
        vertices, triangles = filter_mesh(vertices, triangles, keep)
        if vertices.shape[0] == 0 or triangles.shape[0] == 0:
            raise RuntimeError(f"TSDFVolume.extract_mesh: no surface in the volume ({self.frames} frames integrated, "
                               f"{int((self.count >= int(min_count)).sum())} of {self.count.numel()} lattice points observed)")
        return self.to_world(vertices), triangles

    def scene(self, grid_resolution=None, min_count=1):
        """The mesh as a raycast.RaycastingScene in world coordinates."""
        from .raycast import RaycastingScene
        vertices, triangles = self.extract_mesh(min_count)
        return RaycastingScene(vertices, triangles, grid_resolution=grid_resolution)
