"""Exact k-nearest neighbours of a point cloud on the device (csrc/knn.hip, include/lidarnerf_hip.h lnh_knn_*): what
lidarnvs/lidarnvs_meshing.py does in predict_frame with Open3D's KDTreeFlann (search_knn_vector_3d, one Python iteration per hit
point) and np.mean over the neighbours' intensities — with every array kept on the GPU.

The distance is d2 = ((dx dx) + (dy dy)) + (dz dz) in a fixed fp32 operation order; the answer for a query is the min(k, N)
smallest (d2, point index) pairs over ALL points whatever the grid resolution.  The tie rule (smallest index) and the
fp64 rank-order mean are this package's own: there is no Open3D here to pin them against.  No CPU fallback."""
import numpy as np
import torch

from . import _hip
from ._cellgrid import MAX_CELLS_PER_AXIS, cubic_cells, device as _device, grid_triple

_SYMBOLS = ("lnh_knn_workspace_size", "lnh_knn_bounds", "lnh_knn_build_count", "lnh_knn_build_fill", "lnh_knn_search")
MAX_K = 16                 # kKnnMaxK
# the default grid (tools/bench_knn.py sweeps it, profiles/knn_bench.txt): points per cell, cubic cells.  A finer grid costs
# 4 bytes per cell next to the 28 bytes per point of the cloud and its sorted copy.
DEFAULT_POINTS_PER_CELL = 1.0


def default_grid_resolution(n_points, box):
    """The rule behind grid_resolution=None: about DEFAULT_POINTS_PER_CELL points per cell, cubic cells as far as the limit of
    1 ... 1024 cells per axis allows; an axis without extent gets the kernel's floored width (largest extent / 1024).  A speed
    choice, not a contract: every grid gives the same answer.  box: the six numbers lo[3], hi[3]."""
    _, _, ext, side = cubic_cells(box, float(n_points) / DEFAULT_POINTS_PER_CELL)
    return tuple(max(1, min(int(round(ext[a] / side)), MAX_CELLS_PER_AXIS)) for a in range(3))


def _cloud(points):
    """Shape and type checks that need no device; returns the cloud as a torch tensor (wherever it lives)."""
    p = torch.from_numpy(np.ascontiguousarray(points)) if isinstance(points, np.ndarray) else points
    if not torch.is_tensor(p):
        raise TypeError("PointCloudIndex: points must be a tensor or a NumPy array")
    if p.dim() != 2 or p.shape[1] != 3 or not p.is_floating_point():
        raise ValueError(f"PointCloudIndex: points must be a float [N, 3] array, got {p.dtype} {tuple(p.shape)}")
    if p.shape[0] == 0:
        raise ValueError("PointCloudIndex: empty cloud (0 points)")
    if p.shape[0] >= 1 << 31:
        raise ValueError("PointCloudIndex: indices are int32: fewer than 2^31 points")
    return p


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"lidarnerf.knn: k must be an int in 1 ... {MAX_K}, got {k!r}")
    return int(k)


def check_queries(queries):
    """The queries as a contiguous float32 [Q,3] GPU tensor.  A CPU tensor or a NumPy array is refused: the hit points of a
    frame are made on the device (no CPU fallback)."""
    if not torch.is_tensor(queries) or not queries.is_cuda:
        raise RuntimeError("lidarnerf.knn: queries must be a tensor on the GPU (no CPU fallback)")
    if queries.dim() != 2 or queries.shape[1] != 3 or not queries.is_floating_point():
        raise ValueError(f"lidarnerf.knn: queries must be a float [Q, 3] tensor, got {queries.dtype} {tuple(queries.shape)}")
    if queries.shape[0] >= 1 << 31:
        raise ValueError("lidarnerf.knn: at most 2^31 - 1 queries per call")
    return queries.detach().float().contiguous()


def _check_valid(valid, Q, device):
    if valid is None:
        return None
    if not torch.is_tensor(valid) or not valid.is_cuda:
        raise RuntimeError("lidarnerf.knn: valid must be a tensor on the GPU (no CPU fallback)")
    if valid.dtype not in (torch.bool, torch.uint8) or valid.dim() != 1 or valid.shape[0] != Q:
        raise ValueError(f"lidarnerf.knn: valid must be a bool / uint8 [{Q}] tensor, got {valid.dtype} {tuple(valid.shape)}")
    if valid.device != device:
        raise RuntimeError(f"lidarnerf.knn: valid on {valid.device}, the cloud on {device}")
    valid = valid.detach().contiguous()
    return valid.view(torch.uint8) if valid.dtype == torch.bool else valid


class PointCloudIndex:
    """points float [N,3] (a tensor or a NumPy array; kept on the GPU as float32).  grid_resolution: None
    (default_grid_resolution), an int or (nx, ny, nz).  The build reads the device once — the box with the count of non-finite
    coordinates — and is refused while a stream is capturing."""

    def __init__(self, points, grid_resolution=None):
        p = _cloud(points)
        grid = None if grid_resolution is None else grid_triple(grid_resolution, "PointCloudIndex")
        dev = p.device if p.is_cuda else _device()
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("PointCloudIndex: not while a stream is capturing (the build reads the box back)")
        _hip.require_symbols(_SYMBOLS, "nearest-neighbour search")
        self.points = p.detach().to(dev, torch.float32).contiguous()
        N = self.N = int(self.points.shape[0])
        L = _hip.lib()
        with torch.cuda.device(dev):
            self.box = torch.empty(8, dtype=torch.float32, device=dev)
            ws = torch.empty(max(int(L.lnh_knn_workspace_size(N, 1, 1, 1)), 16), dtype=torch.uint8, device=dev)
            _hip.call("lnh_knn_bounds", self.points.data_ptr(), N, ws.data_ptr(), ws.numel(), self.box.data_ptr())
            words = self.box.view(torch.int32).tolist()  # the one host read
            bad = words[6] & 0xffffffff
            if bad:
                raise ValueError(f"PointCloudIndex: {bad} point coordinates are not finite")
            box = np.array(words[:6], np.int32).view(np.float32).tolist()
            self.grid = default_grid_resolution(N, box) if grid is None else grid
            nx, ny, nz = self.grid
            need = int(L.lnh_knn_workspace_size(N, nx, ny, nz))
            if need > ws.numel():
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self.cell_start = torch.empty(nx * ny * nz + 1, dtype=torch.int32, device=dev)
            self.slabs = torch.empty(2 * (nx + ny + nz), dtype=torch.float32, device=dev)
            self.sorted = torch.empty((N, 4), dtype=torch.float32, device=dev)
            _hip.call("lnh_knn_build_count", self.points.data_ptr(), N, self.box.data_ptr(), nx, ny, nz, ws.data_ptr(), ws.numel(),
                      self.cell_start.data_ptr(), self.slabs.data_ptr())
            _hip.call("lnh_knn_build_fill", self.points.data_ptr(), N, self.box.data_ptr(), nx, ny, nz, ws.data_ptr(), ws.numel(),
                      self.cell_start.data_ptr(), self.sorted.data_ptr())
        self.device = dev
        self.bounds = (tuple(box[:3]), tuple(box[3:6]))

    def _search(self, queries, k, valid, values, want_lists):
        q = check_queries(queries)
        k = _check_k(k)
        if q.device != self.device:
            raise RuntimeError(f"PointCloudIndex: queries on {q.device}, the cloud on {self.device}")
        Q = int(q.shape[0])
        valid = _check_valid(valid, Q, self.device)
        with torch.cuda.device(self.device):
            indices = torch.empty((Q, k), dtype=torch.int32, device=self.device) if want_lists else None
            dist2 = torch.empty((Q, k), dtype=torch.float32, device=self.device) if want_lists else None
            mean = torch.empty(Q, dtype=torch.float32, device=self.device) if values is not None else None
            if Q:
                nx, ny, nz = self.grid
                _hip.call("lnh_knn_search", self.points.data_ptr(), self.N, self.box.data_ptr(), nx, ny, nz,
                          self.cell_start.data_ptr(), self.sorted.data_ptr(), self.slabs.data_ptr(), q.data_ptr(), _hip.ptr(valid), Q,
                          k, _hip.ptr(values), _hip.ptr(indices), _hip.ptr(dist2), _hip.ptr(mean))
        return indices, dist2, mean

    def search_knn(self, queries, k, valid=None):
        """queries float [Q,3] on the GPU, 1 <= k <= 16, valid: optional bool / uint8 [Q] (0 skips the query).  Returns
        (indices i32 [Q,k], dist2 f32 [Q,k]): nearest first, among equal distances the smallest index; -1 / +inf behind the
        min(k, N)-th rank, for a skipped query and for a query with a non-finite coordinate.  One launch, no host read:
        capturable."""
        indices, dist2, _ = self._search(queries, k, valid, None, True)
        return indices, dist2

    def mean_of_neighbours(self, queries, values, k, valid=None):
        """f32 [Q]: the mean of values [N] over the k nearest neighbours of every query (summed in rank order in fp64, divided
        by their number, rounded once to fp32); 0 for a skipped query.  One launch, no host read: capturable."""
        if not torch.is_tensor(values) or not values.is_cuda:
            raise RuntimeError("lidarnerf.knn: values must be a tensor on the GPU (no CPU fallback)")
        if values.numel() != self.N or not values.is_floating_point():
            raise ValueError(f"PointCloudIndex.mean_of_neighbours: values must be {self.N} floats (one per point), got "
                             f"{values.dtype} {tuple(values.shape)}")
        if values.device != self.device:
            raise RuntimeError(f"PointCloudIndex: values on {values.device}, the cloud on {self.device}")
        values = values.detach().reshape(-1).float().contiguous()
        return self._search(queries, k, valid, values, False)[2]
