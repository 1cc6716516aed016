"""Mesh export of the reference Trainer (lidarnerf/nerf/utils.py:139-184 extract_fields / extract_geometry, 1011-1040
save_mesh) with the volume kept on the device: the density lattice goes through model.density (the grid and MLP kernels that
exist) chunk by chunk into one [R, R, R] tensor, marching cubes runs there (csrc/mesh.hip: count, one host read of the two
counts, exact allocation, emit), and the PLY file is written with NumPy.  The reference copies eight chunks to the host, runs
PyMCubes on the CPU and exports through trimesh.  Triangle order and the choice on ambiguous cells are this package's own
(csrc/gen_mc_tables.py), not PyMCubes'; the vertex set is the same."""
import os

import numpy as np
import torch

from .. import _hip

_SYMBOLS = ("lnh_marching_cubes_count", "lnh_marching_cubes_emit", "lnh_marching_cubes_workspace_size")


def _fields(bound_min, bound_max, resolution, query_func, S, device):
    """extract_fields with the volume left on the device: the reference's lattice (torch.linspace per axis, on the host as the
    reference builds it, walked in split(S) chunks with indexing="ij"); every chunk's points are handed to query_func ON the
    device, and its [n] result is stored into the fp32 volume there."""
    R = int(resolution)
    axes = [torch.linspace(float(bound_min[a]), float(bound_max[a]), R).to(device).split(S) for a in range(3)]
    u = torch.empty((R, R, R), dtype=torch.float32, device=device)
    with torch.no_grad():
        for xi, xs in enumerate(axes[0]):
            for yi, ys in enumerate(axes[1]):
                for zi, zs in enumerate(axes[2]):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = query_func(pts)
                    if not torch.is_tensor(val) or not val.is_cuda:
                        raise RuntimeError("lidarnerf.nerf.mesh: query_func must return a tensor on the GPU (no CPU fallback)")
                    u[xi * S:xi * S + len(xs), yi * S:yi * S + len(ys), zi * S:zi * S + len(zs)] = \
                        val.detach().reshape(len(xs), len(ys), len(zs))
    return u


def _device_of(*candidates):
    for c in candidates:
        if torch.is_tensor(c) and c.is_cuda:
            return c.device
    if not torch.cuda.is_available():
        raise RuntimeError("lidarnerf.nerf.mesh: the volume lives on the GPU and none is available (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def density_volume(model, resolution, S=128, fp16=True, *, amp_dtype=torch.float16):
    """fp32 [R, R, R] on the model's device: model.density(pts)["sigma"] on the lattice of model.aabb_infer, under no_grad
    and autocast(enabled=fp16).  No host copy of a chunk, no kernel of its own."""
    box = model.aabb_infer
    if not box.is_cuda:
        raise RuntimeError("lidarnerf.nerf.mesh.density_volume: the model must live on the GPU (no CPU fallback)")
    lo_hi = box.detach().float().cpu().tolist()  # (six numbers; the reference reads them the same way)

    def query_func(pts):
        with torch.autocast("cuda", dtype=amp_dtype, enabled=bool(fp16)):
            return model.density(pts)["sigma"]

    return _fields(lo_hi[:3], lo_hi[3:], resolution, query_func, int(S), box.device)


def marching_cubes(volume, threshold):
    """(vertices [V,3] fp32 in index units, triangles [T,3] int32) on the volume's device (include/lidarnerf_hip.h,
    lnh_marching_cubes_*).  Raises on a CPU tensor and on a volume with a non-finite sample."""
    if not torch.is_tensor(volume) or not volume.is_cuda:
        raise RuntimeError("lidarnerf.nerf.mesh.marching_cubes: the volume must be a tensor on the GPU (no CPU fallback)")
    if volume.dim() != 3:
        raise ValueError(f"marching_cubes: expected an [nx, ny, nz] volume, got {tuple(volume.shape)}")
    _hip.require_symbols(_SYMBOLS, "mesh export")
    vol = volume.detach().float().contiguous()
    nx, ny, nz = vol.shape
    iso = float(threshold)
    with torch.cuda.device(vol.device):
        need = int(_hip.lib().lnh_marching_cubes_workspace_size(nx, ny, nz))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=vol.device)  # (a refused size: the call says why)
        counts = torch.empty(4, dtype=torch.int32, device=vol.device)
        _hip.call("lnh_marching_cubes_count", vol.data_ptr(), nx, ny, nz, iso, ws.data_ptr(), ws.numel(), counts.data_ptr())
        V, T, bad, _ = (c & 0xffffffff for c in counts.tolist())  # the one host read
        if bad:
            raise RuntimeError(f"marching_cubes: {bad} of the volume's {nx * ny * nz} samples are not finite")
        if V >= 1 << 31 or T >= 1 << 31:
            raise RuntimeError(f"marching_cubes: {V} vertices / {T} triangles (0xffffffff: more than 32 bits hold) do not fit "
                               "int32 indices")
        vertices = torch.empty((V, 3), dtype=torch.float32, device=vol.device)
        triangles = torch.empty((T, 3), dtype=torch.int32, device=vol.device)
        if V:
            _hip.call("lnh_marching_cubes_emit", vol.data_ptr(), nx, ny, nz, iso, ws.data_ptr(), ws.numel(),
                      vertices.data_ptr(), V, triangles.data_ptr(), T)
    return vertices, triangles


def extract_fields(bound_min, bound_max, resolution, query_func, S=128):
    """The reference's function (utils.py:139-166): NumPy float32 [R, R, R].  query_func receives its points on the GPU."""
    return _fields(bound_min, bound_max, resolution, query_func, S, _device_of(bound_min, bound_max)).cpu().numpy()


def _to_world(vertices, bound_min, bound_max, resolution):
    """Index units -> the box, in float64 as the reference does it on PyMCubes' float64 vertices (utils.py:177-183)."""
    as_np = lambda b: b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float32)
    b_min_np, b_max_np = as_np(bound_min), as_np(bound_max)
    return vertices.astype(np.float64) / (resolution - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :]


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func):
    """The reference's function (utils.py:169-184): (vertices float64 [V,3] in the box, triangles int32 [T,3]) as NumPy.  The
    volume stays on the device between the two halves."""
    u = _fields(bound_min, bound_max, resolution, query_func, 128, _device_of(bound_min, bound_max))
    vertices, triangles = marching_cubes(u, threshold)
    return _to_world(vertices.cpu().numpy(), bound_min, bound_max, resolution), triangles.cpu().numpy()


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: `float x y z` per vertex, `list uchar int vertex_indices` per face."""
    v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    faces = np.empty(len(t), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    faces["n"], faces["idx"] = 3, t
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """(vertices float32 [V,3], triangles int32 [T,3]) of a file in exactly the format write_ply writes."""
    with open(path, "rb") as f:
        data = f.read()
    head, sep, body = data.partition(b"end_header\n")
    lines = head.decode("ascii", "replace").split("\n")
    if not sep or lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"read_ply: {path} is not a binary little-endian PLY file")
    if [ln for ln in lines if ln.startswith("property")] != ["property float x", "property float y", "property float z",
                                                             "property list uchar int vertex_indices"]:
        raise ValueError(f"read_ply: {path} does not have the properties write_ply writes (float x y z, list uchar int "
                         "vertex_indices)")
    try:
        nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
        nf = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    except (StopIteration, ValueError):
        raise ValueError(f"read_ply: {path} lacks the vertex / face element lines") from None
    if len(body) != nv * 12 + nf * 13:
        raise ValueError(f"read_ply: {path} holds {len(body)} bytes of data, {nv} vertices and {nf} triangles need "
                         f"{nv * 12 + nf * 13}")
    vertices = np.frombuffer(body, "<f4", nv * 3).reshape(nv, 3).astype(np.float32)
    faces = np.frombuffer(body, np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), nf, offset=nv * 12)
    if nf and not (faces["n"] == 3).all():
        raise ValueError(f"read_ply: {path} holds a face that is not a triangle")
    return vertices, faces["idx"].astype(np.int32).reshape(nf, 3)


def _trainer_mesh(trainer, resolution, threshold, ema):
    """(vertices [V,3] fp32 in index units, triangles [T,3] int32) of the trainer's density field, on the device."""
    import contextlib
    model = trainer.model
    use_ema = bool(ema) and trainer.ema is not None
    trainer.gather_table_state()  # (sharded table optimizer: density reads the fp32 table; collective there, a no-op elsewhere)
    with (trainer.ema_weights() if use_ema else contextlib.nullcontext()):
        u = density_volume(model, resolution, fp16=trainer.fp16, amp_dtype=trainer.amp_dtype)
    return marching_cubes(u, threshold)


def to_world_device(vertices, box, resolution):
    """_to_world on the device: the same float64 operations in the same order, rounded to float32 as write_ply rounds them."""
    box = box.detach().to(vertices.device, torch.float32)
    b_min, b_max = box[:3], box[3:]
    world = vertices.double() / (resolution - 1.0) * (b_max - b_min)[None, :].double() + b_min[None, :].double()
    return world.float()


def save_mesh(trainer, save_path, resolution=256, threshold=10, ema=True):
    """LidarTrainer.save_mesh: the density volume of the model (of its averaged weights with `ema` and a trainer that keeps an
    average), marching cubes at `threshold`, vertices mapped into aabb_infer, a PLY file.  Returns (n_vertices, n_triangles)."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("LidarTrainer.save_mesh: not while a stream is capturing (it reads counts back)")
    directory = os.path.dirname(os.path.abspath(save_path))
    os.makedirs(directory, exist_ok=True)
    vertices, triangles = _trainer_mesh(trainer, resolution, threshold, ema)
    box = trainer.model.aabb_infer
    world = _to_world(vertices.cpu().numpy(), box[:3], box[3:], resolution)
    write_ply(save_path, world, triangles.cpu().numpy())
    return int(vertices.shape[0]), int(triangles.shape[0])


def mesh_scene(trainer, resolution=256, threshold=10, ema=True, grid_resolution=None):
    """LidarTrainer.mesh_scene: save_mesh's mesh without the file, as a lidarnerf.raycast.RaycastingScene in world
    coordinates.  The vertices are what read_ply returns from save_mesh's file, bit for bit."""
    from ..raycast import RaycastingScene
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("LidarTrainer.mesh_scene: not while a stream is capturing (it reads counts back)")
    vertices, triangles = _trainer_mesh(trainer, resolution, threshold, ema)
    return RaycastingScene(to_world_device(vertices, trainer.model.aabb_infer, resolution), triangles,
                           grid_resolution=grid_resolution)
