"""Mesh ray casting without a GPU: the entry points exported, declared and bound, every refusal before any launch, the Python
surface with its refusals, the PLY reader, and the CONTRACT ITSELF — the NumPy restatement (tests/raycast_ref.py) of the
watertight intersection function is watertight on a closed marching-cubes mesh where plain Moeller-Trumbore is not, places
its hits on the surface, breaks ties by index and never hits a triangle with two equal vertices.

Zero-area triangles: the ones with a repeated vertex are provably never hit (two sheared vertices coincide, so one edge
function is exactly 0, the float64 recomputation makes the other two exact opposites and det is exactly 0).  Three distinct
collinear vertices are sheared with rounding like any others and carry no such proof; the contract answers a winner whose
normal has no length with a zero normal."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import marching_cubes_ref as mc
import raycast_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2
NAMES = ("lnh_raycast_workspace_size", "lnh_raycast_bounds", "lnh_raycast_build_count", "lnh_raycast_build_fill",
         "lnh_raycast_cast")
SPHERE_ORIGIN = np.array([11.37, 11.9, 12.21], np.float32)
SPHERE_RADIUS = 8.3


# -------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_declared_and_bound():
    from lidarnerf import _hip
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    L = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(L, name), name
        assert re.search(r"LNH_API (int|uint64_t) " + name + r"\(", text), name
        assert name in _hip._OPTIONAL  # detected by symbol: lnh_version() did not move
    assert L.lnh_version() == 102
    assert "Watertight Ray/Triangle Intersection" in text
    assert "Watertight Ray/Triangle Intersection" in open(os.path.join(ROOT, "lidar-nerf_amd", "csrc", "raycast.hip")).read()
    P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
    assert _hip._SIGS["lnh_raycast_bounds"] == [P, U32, P, U32, P, U64, P, P]
    assert _hip._SIGS["lnh_raycast_build_count"] == [P, U32, P, U32, P, U32, U32, U32, P, U64, P, P]
    assert _hip._SIGS["lnh_raycast_build_fill"] == [P, U32, P, U32, P, U32, U32, U32, P, U64, P, P, U64]
    assert _hip._SIGS["lnh_raycast_cast"] == [P, U32, P, U32, P, U32, U32, U32, P, P, U64, P, P, U32, P, P, P, P]
    for name in NAMES[1:]:
        assert getattr(L, name).argtypes == _hip._SIGS[name] + [P]  # the stream comes last
    assert L.lnh_raycast_workspace_size.restype is U64
    assert L.lnh_raycast_workspace_size.argtypes == [U32, U32, U32, U32, U32, U64]


def test_workspace_size():
    from lidarnerf import _hip
    size = _hip.lib().lnh_raycast_workspace_size
    assert size(3, 1, 1, 1, 1, 0) > 0 and size(3, 1, 1, 1, 1, 0) % 16 == 0
    assert size(100, 100, 16, 16, 16, 0) >= 4 * 16 ** 3
    assert size(100, 100, 17, 16, 16, 0) > size(100, 100, 16, 16, 16, 0)
    assert size(100, 100, 1024, 1024, 2, 0) >= 4 * 1024 * 1024 * 2
    for args in ((0, 1, 1, 1, 1, 0), (3, 0, 1, 1, 1, 0), (1 << 31, 1, 1, 1, 1, 0), (3, 1 << 31, 1, 1, 1, 0), (3, 1, 0, 1, 1, 0),
                 (3, 1, 1, 1025, 1, 0), (3, 1, 1, 1, 0xffffffff, 0), (3, 1, 1, 1, 1, 1 << 31)):
        assert size(*args) == 0, args


def test_every_refusal_comes_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced or a kernel is launched
    need = L.lnh_raycast_workspace_size(10, 20, 4, 5, 6, 0)

    def bounds(v=x, V=10, t=x, T=20, ws=x, wsb=need, box=x, counts=x):
        if wsb == need - 4:
            wsb = L.lnh_raycast_workspace_size(V, T, 1, 1, 1, 0) - 4  # (the bounds pass needs what a 1 x 1 x 1 grid needs)
        return L.lnh_raycast_bounds(v, V, t, T, ws, wsb, box, counts, None)

    def count(v=x, V=10, t=x, T=20, box=x, grid=(4, 5, 6), ws=x, wsb=need, cs=x, counts=x):
        return L.lnh_raycast_build_count(v, V, t, T, box, *grid, ws, wsb, cs, counts, None)

    def fill(v=x, V=10, t=x, T=20, box=x, grid=(4, 5, 6), ws=x, wsb=need, cs=x, ct=x, entries=50):
        return L.lnh_raycast_build_fill(v, V, t, T, box, *grid, ws, wsb, cs, ct, entries, None)

    def cast(v=x, V=10, t=x, T=20, box=x, grid=(4, 5, 6), cs=x, ct=x, entries=50, o=x, d=x, N=7, th=x, ids=x, nrm=x, inc=x):
        return L.lnh_raycast_cast(v, V, t, T, box, *grid, cs, ct, entries, o, d, N, th, ids, nrm, inc, None)

    mesh = ((dict(v=None), INVALID_ARG, "null"), (dict(t=None), INVALID_ARG, "null"), (dict(V=0), INVALID_ARG, "empty mesh"),
            (dict(T=0), INVALID_ARG, "empty mesh"), (dict(V=1 << 31), UNSUPPORTED, "int32"), (dict(T=1 << 31), UNSUPPORTED, "int32"))
    grid = ((dict(box=None), INVALID_ARG, "null"), (dict(grid=(0, 5, 6)), INVALID_ARG, ">= 1"), (dict(grid=(4, 5, 0)), INVALID_ARG, ">= 1"),
            (dict(grid=(4, 1025, 6)), UNSUPPORTED, "1024"))
    work = ((dict(ws=None), INVALID_ARG, "workspace"), (dict(wsb=need - 4), INVALID_ARG, "workspace"), (dict(ws=18), INVALID_ARG, "workspace"))
    lists = ((dict(cs=None), INVALID_ARG, "null"), (dict(ct=None), INVALID_ARG, "null"), (dict(entries=0), INVALID_ARG, "entries"),
             (dict(entries=1 << 31), UNSUPPORTED, "2^31 - 1"))
    cases = ((bounds, mesh + work + ((dict(box=None), INVALID_ARG, "null"), (dict(counts=None), INVALID_ARG, "null"))),
             (count, mesh + grid + work + ((dict(grid=(4, 5, 7)), INVALID_ARG, "workspace"), (dict(cs=None), INVALID_ARG, "null"),
                                           (dict(counts=None), INVALID_ARG, "null"))),
             (fill, mesh + grid + work + lists),
             (cast, mesh + grid + lists + ((dict(o=None), INVALID_ARG, "null"), (dict(d=None), INVALID_ARG, "null"),
                                           (dict(th=None), INVALID_ARG, "null"), (dict(ids=None), INVALID_ARG, "null"),
                                           (dict(nrm=None), INVALID_ARG, "null"), (dict(N=1 << 31), UNSUPPORTED, "rays"))))
    for fn, rows in cases:
        for kw, code, word in rows:
            assert fn(**kw) == code and word in err(), (fn.__name__, kw, err())
    assert "coarser grid" in (fill(entries=1 << 31), err())[1]
    assert cast(N=0, o=None, d=None, th=None, ids=None, nrm=None) == 0  # no rays: nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------------ the Python side
def test_python_surface_and_refusals_that_need_no_device(tmp_path):
    from lidarnerf import raycast
    from lidarnerf.nerf import mesh
    from lidarnerf.nerf.train_step import LidarTrainer
    Scene = raycast.RaycastingScene
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(Scene.__init__) == ["self", "vertices", "triangles", "grid_resolution"]
    assert inspect.signature(Scene.__init__).parameters["grid_resolution"].default is None
    assert names(Scene.cast_rays)[:3] == ["self", "rays", "rays_d"] and names(Scene.intersect_rays)[:2] == ["self", "rays"]
    assert names(Scene.intersect_lidar) == ["self", "lidar_K", "lidar_pose", "lidar_H", "lidar_W"]
    assert names(Scene.raydrop_features) == ["self", "lidar_K", "lidar_pose", "lidar_H", "lidar_W", "intensities"]
    assert names(Scene.from_ply)[0] == "path" and names(mesh.read_ply) == ["path"]
    sig = inspect.signature(LidarTrainer.mesh_scene)
    assert list(sig.parameters) == ["self", "resolution", "threshold", "ema", "grid_resolution"]
    assert [sig.parameters[k].default for k in ("resolution", "threshold", "ema", "grid_resolution")] == [256, 10, True, None]
    v, t = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    for bad_v, bad_t in ((np.zeros((4, 2), np.float32), t), (np.zeros(12, np.float32), t), (np.zeros((4, 3), np.int32), t),
                         (v, np.zeros((2, 4), np.int32)), (v, np.zeros((2, 3), np.float32)), (v, np.zeros((2, 3), bool)),
                         (np.zeros((0, 3), np.float32), t), (v, np.zeros((0, 3), np.int32))):
        with pytest.raises(ValueError, match="must be|empty mesh"):
            Scene(bad_v, bad_t)
    with pytest.raises(ValueError, match="empty mesh"):
        Scene(torch.zeros(0, 3), torch.zeros((0, 3), dtype=torch.int64))
    with pytest.raises(TypeError):
        Scene([[0.0, 0, 0]], t)
    for grid in (0, -1, 1025, (1, 2), (1, 2, 0), (1, 2, 3.5), "8", True, (4, 4, 2000)):
        with pytest.raises(ValueError, match="grid_resolution"):
            Scene(v, t, grid_resolution=grid)
    # rays: a CPU tensor or a NumPy array is refused with the package's wording, whatever the scene
    for rays in (torch.zeros(5, 6), np.zeros((5, 6), np.float32)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            raycast.split_rays(rays)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raycast.split_rays(torch.zeros(5, 3), torch.zeros(5, 3))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Scene(v, t)
        path = os.path.join(tmp_path, "tri.ply")
        mesh.write_ply(path, np.eye(3), np.array([[0, 1, 2]], np.int32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Scene.from_ply(path)


def test_default_grid_resolution_rule():
    from lidarnerf.raycast import MAX_CELLS_PER_AXIS, default_grid_resolution as rule
    cube = [0, 0, 0, 1, 1, 1]
    assert rule(1, cube) == (1, 1, 1) and rule(8, cube) == (2, 2, 2) and rule(1000, cube) == (10, 10, 10)
    assert rule(10 ** 12, cube) == (MAX_CELLS_PER_AXIS,) * 3
    nx, ny, nz = rule(4000, [0, 0, 0, 4, 2, 1])
    assert nx > ny > nz >= 1 and abs(nx * ny * nz - 4000) < 1500  # the proportions of the box
    assert rule(1000, [0, 0, 0, 1, 1, 0])[2] == 1 and rule(50, [0, 0, 0, 0, 0, 0]) == (4, 4, 4)  # a flat mesh, a single point
    assert rule(50, [2, 2, 2, 2, 2, 2]) == (1, 1, 1)  # ... away from zero: the precision limit
    # a box far from zero: no finer than the walk's arithmetic resolves (extent * 2^11 / |coordinate|)
    far = rule(10 ** 6, [1000, 1000, 1000, 1001, 1001, 1001])
    assert far == (2, 2, 2)
    assert all(1 <= n <= MAX_CELLS_PER_AXIS for n in far + rule(10 ** 9, [-1, -1, -1, 1, 1, 1]))


def test_read_ply_reads_what_write_ply_writes(tmp_path):
    from lidarnerf.nerf import mesh
    vol, iso = mc.sphere_volume((9, 10, 11), 3.2)
    v, t, _ = mc.marching_cubes(vol, iso)
    path = os.path.join(tmp_path, "sphere.ply")
    world = v.astype(np.float64) * 0.37 - 1.0
    mesh.write_ply(path, world, t)
    got_v, got_t = mesh.read_ply(path)
    assert got_v.dtype == np.float32 and got_t.dtype == np.int32 and got_v.shape == v.shape and got_t.shape == t.shape
    assert np.array_equal(got_v.view(np.int32), world.astype(np.float32).view(np.int32)) and np.array_equal(got_t, t)
    want_v, want_t = mc.read_ply(path)  # the tests' own parser
    assert np.array_equal(got_v.view(np.int32), want_v.view(np.int32)) and np.array_equal(got_t, want_t)
    mesh.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    got_v, got_t = mesh.read_ply(path)
    assert got_v.shape == (0, 3) and got_t.shape == (0, 3)
    data = open(path, "rb").read()
    for broken in (data.replace(b"binary_little_endian", b"ascii"), data.replace(b"property float z\n", b""), data + b"\0",
                   data.replace(b"end_header\n", b"")):
        with open(path, "wb") as f:
            f.write(broken)
        with pytest.raises(ValueError, match="read_ply"):
            mesh.read_ply(path)


# ------------------------------------------------------------------------------------------------------- the contract
@functools.lru_cache(maxsize=None)
def _sphere():
    vol, iso = mc.sphere_volume((24, 24, 24), SPHERE_RADIUS)
    v, t, _ = mc.marching_cubes(vol, iso)
    assert (len(v), len(t)) == (1300, 2596) and mc.open_edges(t) == []
    o, d = rr.rays_at_features(v, t, SPHERE_ORIGIN)
    assert len(o) == 1300 + len(rr.mesh_edges(t)) + 2596 + 6
    out = rr.cast_rays(v, t, o, d)
    for a in (v, t, o, d) + tuple(out.values()):
        a.setflags(write=False)
    return v, t, o, d, out


def test_the_restatement_is_watertight_where_moller_trumbore_is_not():
    v, t, o, d, out = _sphere()
    escaped = int((out["primitive_ids"] < 0).sum())
    plain = int((~rr.moller_trumbore_hits(v, t, o, d)).sum())
    print(f"{len(o)} rays from inside the closed mesh: watertight test lets {escaped} escape, Moeller-Trumbore {plain}")
    assert escaped == 0
    assert np.isfinite(out["t_hit"]).all() and (out["t_hit"] > 0).all()
    assert plain > 0  # (what the contract is there for)


def test_every_hit_lies_within_a_cell_diagonal_of_the_sphere():
    v, t, o, d, out = _sphere()
    centre = np.array([(24 - 1) / 2 + 0.13 * (a + 1) for a in range(3)])
    p = o.astype(np.float64) + d.astype(np.float64) * out["t_hit"].astype(np.float64)[:, None]
    off = np.abs(np.linalg.norm(p - centre, axis=1) - SPHERE_RADIUS)
    print("largest distance of a hit from the sphere:", off.max())
    assert off.max() <= np.sqrt(3.0)  # a marching-cubes triangle lives inside one cell
    # the winner is a triangle the ray was aimed at (rays at centroids: that triangle or a nearer one), normals are unit
    n = out["primitive_normals"].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    unit = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    assert np.allclose(out["incidences"], np.abs((d.astype(np.float64) * n).sum(1)), rtol=1e-5, atol=1e-6)
    assert ((unit[:-6] * n[:-6]).sum(1) > 0).all()  # from inside, the outward normals point along the rays


QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)


def test_ties_go_to_the_smaller_index():
    o = np.array([[0.25, 0.25, 1], [0.5, 0.5, 2], [1, 1, 1], [0, 0, 3], [0.75, 0.25, 1], [0.25, 0.75, 1], [2, 2, 1]], np.float32)
    d = np.array([[0, 0, -1]] * 7, np.float32)
    for tris, want in ((np.array([[0, 1, 2], [0, 2, 3]], np.int32), [0, 0, 0, 0, 0, 1, -1]),
                       (np.array([[0, 2, 3], [0, 1, 2]], np.int32), [0, 0, 0, 0, 1, 0, -1])):
        out = rr.cast_rays(QUAD_V, tris, o, d)
        assert out["primitive_ids"].tolist() == want
        assert out["t_hit"].tolist() == [1, 2, 1, 3, 1, 1, np.inf]  # on the shared edge and at both shared vertices: equal t
        hit, _ = rr.intersect(o[:4], d[:4], QUAD_V[tris[:, 0]], QUAD_V[tris[:, 1]], QUAD_V[tris[:, 2]])
        assert hit.all()  # both triangles are hit there: the index decides
        assert np.array_equal(out["primitive_normals"][:6], np.array([[0, 0, 1]] * 6, np.float32))
        assert np.array_equal(out["primitive_normals"][6], np.zeros(3, np.float32)) and out["incidences"].tolist() == [1] * 6 + [0]
    # a duplicated triangle: the first copy
    out = rr.cast_rays(QUAD_V, np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2]], np.int32), o[4:5], d[4:5])
    assert out["primitive_ids"].tolist() == [0]
    # unnormalised directions: t is in units of |d|
    out = rr.cast_rays(QUAD_V, np.array([[0, 1, 2], [0, 2, 3]], np.int32), o[:2], d[:2] * np.float32(4.0))
    assert out["t_hit"].tolist() == [0.25, 0.5] and out["primitive_ids"].tolist() == [0, 0]


def test_triangles_with_a_repeated_vertex_never_hit():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (12, 3)).astype(np.float32)
    tris = np.array([[0, 0, 1], [2, 3, 3], [4, 5, 4], [6, 6, 6], [7, 8, 7], [9, 9, 10]], np.int32)
    targets = np.concatenate([v, (v[tris[:, 0]] + v[tris[:, 1]] + v[tris[:, 2]]) / np.float32(3),
                              (v[tris[:, 0]] + v[tris[:, 2]]) * np.float32(0.5), (v[tris[:, 1]] + v[tris[:, 2]]) * np.float32(0.5)])
    origins = np.array([[0.1, 0.2, 0.3], [3, 2, 1], [0, 0, 0], [-2, 0.5, 0.25]], np.float32)
    o = np.repeat(origins, len(targets), axis=0)
    d = np.tile(targets, (len(origins), 1)) - o
    o = np.concatenate([o, v[tris[:, 0]]])  # origins ON the vertices too
    d = np.concatenate([d, rr.AXES[:len(tris)]])
    out = rr.cast_rays(v, tris, o, d)
    assert (out["primitive_ids"] == -1).all() and np.isinf(out["t_hit"]).all()
    assert not out["primitive_normals"].any() and not out["incidences"].any()
    assert not rr.normals_of(v, tris).any()  # and their normal is the zero vector


def test_rays_that_miss_everything_by_rule():
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    o = np.array([[0.3, 0.3, 1]] * 5 + [[np.nan, 0.3, 1], [0.3, np.inf, 1]], np.float32)
    d = np.array([[0, 0, 0], [0, 0, np.nan], [np.inf, 0, -1], [0, -np.inf, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1]], np.float32)
    out = rr.cast_rays(QUAD_V, tris, o, d)
    assert (out["primitive_ids"] == -1).all()  # zero / NaN / inf direction, pointing away, NaN / inf origin
    assert rr.cast_rays(QUAD_V, tris, o[:1], np.array([[0, 0, -1]], np.float32))["primitive_ids"].tolist() == [0]
