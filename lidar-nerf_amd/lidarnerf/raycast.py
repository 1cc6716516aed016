"""Closest-hit ray casting against a triangle mesh on the device (csrc/raycast.hip, include/lidarnerf_hip.h lnh_raycast_*):
what lidarnvs/lidarnvs_meshing.py does with Open3D's RaycastingScene (Embree on the host) — LidarNVSMeshing.intersect_rays,
intersect_lidar and the 10-channel image of predict_frame_with_raydrop — with every array kept on the GPU.

The intersection test is the watertight one (Woop, Benthin, Wald 2013) in a fixed fp32 operation order; the answer for a ray is
the minimum of (t, triangle index) over ALL triangles whatever the grid resolution.  The orientation of the normal
(cross(v1 - v0, v2 - v0), not flipped towards the ray) and the tie rule (smallest index) are this package's own: there is no
Open3D here to pin them against.  No CPU fallback."""
import math

import numpy as np
import torch

from . import _hip
from ._cellgrid import MAX_CELLS_PER_AXIS, cubic_cells, device as _device, grid_triple

_SYMBOLS = ("lnh_raycast_workspace_size", "lnh_raycast_bounds", "lnh_raycast_build_count", "lnh_raycast_build_fill",
            "lnh_raycast_cast")
MAX_ENTRIES = (1 << 31) - 1
# the default grid (tools/bench_raycast.py chose it, profiles/raycast_bench.txt): cells per triangle, spread over the axes in
# the proportions of the box
DEFAULT_CELLS_PER_TRIANGLE = 1.0


def default_grid_resolution(n_triangles, box):
    """The rule behind grid_resolution=None: about DEFAULT_CELLS_PER_TRIANGLE cells per triangle, cubic cells as far as the
    limits allow — 1 ... 1024 cells per axis, and a cell no finer than the walk's arithmetic resolves at the distance of the box
    from zero (n <= extent * 2^11 / largest |coordinate|; the kernel falls back to all triangles for a ray it cannot walk, a
    finer grid would only make every ray do so).  box: the six numbers lo[3], hi[3]."""
    lo, hi, ext, side = cubic_cells(box, DEFAULT_CELLS_PER_TRIANGLE * float(n_triangles))
    mag = max(float(np.abs(lo).max()), float(np.abs(hi).max()), 1e-30)
    out = []
    for a in range(3):
        n = int(round(ext[a] / side))
        n = min(n, int(ext[a] * 2048.0 / mag), MAX_CELLS_PER_AXIS)
        out.append(max(n, 1))
    return tuple(out)


def _mesh_arrays(vertices, triangles):
    """Shape and type checks that need no device; returns the two arrays as torch tensors (wherever they live)."""
    v = torch.from_numpy(np.ascontiguousarray(vertices)) if isinstance(vertices, np.ndarray) else vertices
    t = torch.from_numpy(np.ascontiguousarray(triangles)) if isinstance(triangles, np.ndarray) else triangles
    if not torch.is_tensor(v) or not torch.is_tensor(t):
        raise TypeError("RaycastingScene: vertices and triangles must be tensors or NumPy arrays")
    if v.dim() != 2 or v.shape[1] != 3 or not v.is_floating_point():
        raise ValueError(f"RaycastingScene: vertices must be a float [V, 3] array, got {v.dtype} {tuple(v.shape)}")
    if t.dim() != 2 or t.shape[1] != 3 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"RaycastingScene: triangles must be an integer [T, 3] array, got {t.dtype} {tuple(t.shape)}")
    if v.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError(f"RaycastingScene: empty mesh ({v.shape[0]} vertices, {t.shape[0]} triangles)")
    if v.shape[0] >= 1 << 31 or t.shape[0] >= 1 << 31:
        raise ValueError("RaycastingScene: indices are int32: fewer than 2^31 vertices and triangles")
    return v, t


def split_rays(rays, rays_d=None):
    """(rays_o, rays_d) as contiguous float32 [N,3] GPU tensors from `rays` [N,6] or from (rays_o [N,3], rays_d [N,3]).
    A CPU tensor or a NumPy array is refused: the rays of a frame are made on the device (no CPU fallback)."""
    given = (rays,) if rays_d is None else (rays, rays_d)
    for r in given:
        if not torch.is_tensor(r) or not r.is_cuda:
            raise RuntimeError("lidarnerf.raycast: rays must be tensors on the GPU (no CPU fallback)")
        if not r.is_floating_point():
            raise ValueError(f"lidarnerf.raycast: rays must be floating point, got {r.dtype}")
    if rays_d is None:
        if rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError(f"lidarnerf.raycast: rays must be an [N, 6] tensor (origin, direction), got {tuple(rays.shape)}")
        o, d = rays[:, :3], rays[:, 3:]
    else:
        o, d = rays, rays_d
        if o.dim() != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError(f"lidarnerf.raycast: rays_o and rays_d must both be [N, 3], got {tuple(o.shape)} and "
                             f"{tuple(d.shape)}")
    if o.shape[0] >= 1 << 31:
        raise ValueError("lidarnerf.raycast: at most 2^31 - 1 rays per call")
    return o.detach().float().contiguous(), d.detach().float().contiguous()


class RaycastingScene:
    """vertices float [V,3], triangles integer [T,3] (tensors or NumPy arrays; moved to the GPU, float32 / int32).
    grid_resolution: None (default_grid_resolution), an int or (nx, ny, nz).  The build reads the device twice — the box with
    the counts of bad values, then the total length of the cell lists — and is refused while a stream is capturing."""

    def __init__(self, vertices, triangles, grid_resolution=None):
        v, t = _mesh_arrays(vertices, triangles)
        grid = None if grid_resolution is None else grid_triple(grid_resolution, "RaycastingScene")
        dev = v.device if v.is_cuda else (t.device if t.is_cuda else _device())
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("RaycastingScene: not while a stream is capturing (the build reads counts back)")
        _hip.require_symbols(_SYMBOLS, "mesh ray casting")
        self.vertices = v.detach().to(dev, torch.float32).contiguous()
        t = t.detach().to(dev)
        if t.dtype in (torch.int64, torch.uint32, torch.uint64):
            t = t.to(torch.int64).clamp(-1, (1 << 31) - 1)  # (an index int32 cannot hold stays out of range: the build counts it)
        self.triangles = t.to(torch.int32).contiguous()
        V, T = int(self.vertices.shape[0]), int(self.triangles.shape[0])
        self.V, self.T = V, T
        L = _hip.lib()
        with torch.cuda.device(dev):
            self.box = torch.empty(9, dtype=torch.float32, device=dev)
            self.counts = torch.empty(4, dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(L.lnh_raycast_workspace_size(V, T, 1, 1, 1, 0)), 16), dtype=torch.uint8, device=dev)
            _hip.call("lnh_raycast_bounds", self.vertices.data_ptr(), V, self.triangles.data_ptr(), T, ws.data_ptr(), ws.numel(),
                      self.box.data_ptr(), self.counts.data_ptr())
            box = self.box.tolist()  # host read 1 (the counts ride on the same synchronisation)
            bad_coords, bad_indices = (c & 0xffffffff for c in self.counts.tolist()[:2])
            if bad_coords:
                raise ValueError(f"RaycastingScene: {bad_coords} vertex coordinates are not finite")
            if bad_indices:
                raise ValueError(f"RaycastingScene: {bad_indices} triangle indices are outside [0, {V})")
            self.grid = default_grid_resolution(T, box) if grid is None else grid
            nx, ny, nz = self.grid
            cells = nx * ny * nz
            need = int(L.lnh_raycast_workspace_size(V, T, nx, ny, nz, 0))
            if need > ws.numel():
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self.cell_start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
            _hip.call("lnh_raycast_build_count", self.vertices.data_ptr(), V, self.triangles.data_ptr(), T, self.box.data_ptr(),
                      nx, ny, nz, ws.data_ptr(), ws.numel(), self.cell_start.data_ptr(), self.counts.data_ptr())
            lo, hi = (c & 0xffffffff for c in self.counts.tolist()[2:])  # host read 2
            self.entries = hi << 32 | lo
            if self.entries > MAX_ENTRIES:
                raise ValueError(f"RaycastingScene: the cell lists of a {nx} x {ny} x {nz} grid would hold {self.entries} entries, "
                                 f"at most {MAX_ENTRIES} fit: use a coarser grid (grid_resolution)")
            self.cell_tris = torch.empty(self.entries, dtype=torch.int32, device=dev)
            _hip.call("lnh_raycast_build_fill", self.vertices.data_ptr(), V, self.triangles.data_ptr(), T, self.box.data_ptr(),
                      nx, ny, nz, ws.data_ptr(), ws.numel(), self.cell_start.data_ptr(), self.cell_tris.data_ptr(), self.entries)
        self.device = dev
        self.bounds = (tuple(box[:3]), tuple(box[3:6]))

    @classmethod
    def from_ply(cls, path, grid_resolution=None):
        """The scene of a file save_mesh wrote (nerf.mesh.read_ply)."""
        from .nerf.mesh import read_ply
        vertices, triangles = read_ply(path)
        return cls(vertices, triangles, grid_resolution=grid_resolution)

    # ---- Open3D's surface
    def cast_rays(self, rays, rays_d=None, incidences=True):
        """rays [N,6] (origin, direction) or (rays_o [N,3], rays_d [N,3]), GPU tensors; directions need not be normalised.
        Returns Open3D's keys as device tensors — t_hit f32 [N] (inf on a miss, in units of |d|), primitive_ids i32 [N] (-1),
        primitive_normals f32 [N,3] (zeros) — plus incidences f32 [N] = |d . n|.  One launch, no host read: capturable."""
        o, d = split_rays(rays, rays_d)
        if o.device != self.device:
            raise RuntimeError(f"RaycastingScene.cast_rays: rays on {o.device}, the scene on {self.device}")
        N = int(o.shape[0])
        with torch.cuda.device(self.device):
            t_hit = torch.empty(N, dtype=torch.float32, device=self.device)
            ids = torch.empty(N, dtype=torch.int32, device=self.device)
            normals = torch.empty((N, 3), dtype=torch.float32, device=self.device)
            inc = torch.empty(N, dtype=torch.float32, device=self.device) if incidences else None
            if N:
                nx, ny, nz = self.grid
                _hip.call("lnh_raycast_cast", self.vertices.data_ptr(), self.V, self.triangles.data_ptr(), self.T, self.box.data_ptr(),
                          nx, ny, nz, self.cell_start.data_ptr(), self.cell_tris.data_ptr(), self.entries, o.data_ptr(), d.data_ptr(),
                          N, t_hit.data_ptr(), ids.data_ptr(), normals.data_ptr(), _hip.ptr(inc))
        out = {"t_hit": t_hit, "primitive_ids": ids, "primitive_normals": normals}
        if incidences:
            out["incidences"] = inc
        return out

    # ---- the reference's surface (lidarnvs/lidarnvs_meshing.py:293-353)
    def intersect_rays(self, rays, rays_d=None):
        """The reference's hit_dict, unfiltered, as device tensors: masks bool [N], depths f32 [N] (inf on a miss), points
        [N,3] = o + d / |d| * depth, normals [N,3]."""
        o, d = split_rays(rays, rays_d)
        hit = self.cast_rays(o, d, incidences=False)
        return self._hit_dict(o, d, hit)

    @staticmethod
    def _hit_dict(o, d, hit):
        depths = hit["t_hit"]
        unit = d / torch.linalg.norm(d, dim=1, keepdim=True)
        return {"masks": depths != math.inf, "depths": depths, "points": o + unit * depths[:, None],
                "normals": hit["primitive_normals"]}

    def lidar_rays(self, lidar_K, lidar_pose, lidar_H, lidar_W):
        """(rays_o, rays_d) [H*W,3] of one frame on the device (lnh_lidar_frame_rays: get_lidar_rays' arithmetic).  lidar_K =
        (fov_up, fov) in degrees, lidar_pose [4,4] lidar -> world."""
        _hip.require_symbols(("lnh_lidar_frame_rays",), "frame rays")
        K = [float(x) for x in (lidar_K.tolist() if hasattr(lidar_K, "tolist") else lidar_K)]
        H, W = int(lidar_H), int(lidar_W)
        if len(K) != 2 or H <= 0 or W <= 0:
            raise ValueError(f"RaycastingScene: lidar_K must be (fov_up, fov) and the frame {H} x {W} must not be empty")
        pose = lidar_pose if torch.is_tensor(lidar_pose) else torch.from_numpy(np.asarray(lidar_pose, np.float32))
        if tuple(pose.shape) != (4, 4):
            raise ValueError(f"RaycastingScene: lidar_pose must be [4, 4], got {tuple(pose.shape)}")
        pose = pose.detach().to(self.device, torch.float32).contiguous()
        with torch.cuda.device(self.device):
            rays_o = torch.empty((H * W, 3), dtype=torch.float32, device=self.device)
            rays_d = torch.empty_like(rays_o)
            _hip.call("lnh_lidar_frame_rays", pose.data_ptr(), 1, 0, H, W, K[0], K[1], rays_o.data_ptr(), rays_d.data_ptr())
        return rays_o, rays_d

    def intersect_lidar(self, lidar_K, lidar_pose, lidar_H, lidar_W):
        """intersect_rays on the rays of one frame."""
        o, d = self.lidar_rays(lidar_K, lidar_pose, lidar_H, lidar_W)
        return self._hit_dict(o, d, self.cast_rays(o, d, incidences=False))

    def raydrop_features(self, lidar_K, lidar_pose, lidar_H, lidar_W, intensities=None):
        """The [1, 10, H, W] image predict_frame_with_raydrop hands the ray-drop U-Net (lidarnvs_meshing.py:198-250): hit mask,
        depth (0 on a miss), normal x 3, incidence |rays_d . normal|, intensity, rays_d x 3.  intensities: [H, W] (or H*W values)
        on the GPU, zeros when not given — the reference's nearest-neighbour lookup of intensities is not part of this."""
        H, W = int(lidar_H), int(lidar_W)
        o, d = self.lidar_rays(lidar_K, lidar_pose, H, W)
        hit = self.cast_rays(o, d)
        mask = hit["t_hit"] != math.inf
        depth = torch.where(mask, hit["t_hit"], torch.zeros_like(hit["t_hit"]))
        if intensities is None:
            inten = torch.zeros_like(depth)
        else:
            if not torch.is_tensor(intensities) or not intensities.is_cuda:
                raise RuntimeError("RaycastingScene.raydrop_features: intensities must be a tensor on the GPU (no CPU fallback)")
            if intensities.numel() != H * W:
                raise ValueError(f"RaycastingScene.raydrop_features: {intensities.numel()} intensities for a {H} x {W} frame")
            inten = intensities.detach().to(torch.float32).reshape(-1)
        images = torch.cat([mask.to(torch.float32)[:, None], depth[:, None], hit["primitive_normals"], hit["incidences"][:, None],
                            inten[:, None], d], dim=1)
        return images.reshape(1, H, W, 10).permute(0, 3, 1, 2)
