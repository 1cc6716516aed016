"""Mesh ray casting on the device (csrc/raycast.hip, lidarnerf/raycast.py, LidarTrainer.mesh_scene) against the NumPy
restatement of its contract (tests/raycast_ref.py).

t_hit and primitive_ids are compared BIT FOR BIT, always: a differing t or id is a bug, never a tolerance.  Normals and
incidences are compared bit for bit too: subtractions, products, one sqrtf and three divisions, each one IEEE fp32 operation on
both sides (hipcc's fp32 division and sqrtf are correctly rounded at the library's flags, nothing is contracted:
-ffp-contract=off).  No tolerance is used anywhere in this file."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import marching_cubes_ref as mc
import raycast_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5ca1ab1e
KEYS = ("t_hit", "primitive_ids", "primitive_normals", "incidences")
RAY_COUNTS = (1, 63, 64, 65, 257, 4099)


def _scan_tile():
    """kScanTile of csrc/scan.h: the cells one tile of the one-workgroup scan covers."""
    text = open(os.path.join(ROOT, "lidar-nerf_amd", "csrc", "scan.h")).read()
    m = re.search(r"kScanThreads = (\d+), kScanPerThread = (\d+), kScanTile = kScanThreads \* kScanPerThread;", text)
    return int(m.group(1)) * int(m.group(2))


PAST_ONE_TILE = (17, 19, 16)  # 5168 cells
ONE_TILE = (16, 16, 16)  # 4096 cells: exactly one tile of the scan
ONE_PAST_A_TILE = (1, 17, 241)  # 4097 cells: the second tile holds one cell
GRIDS = {"all_triangles": (1, 1, 1), "2x3x5": (2, 3, 5), "default": None, "past_one_scan_tile": PAST_ONE_TILE,
         "one_scan_tile": ONE_TILE, "one_past_a_scan_tile": ONE_PAST_A_TILE}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(v, t, grid=None):
    from lidarnerf.raycast import RaycastingScene
    return RaycastingScene(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32), grid_resolution=grid)


def _cast(scene, o, d):
    out = scene.cast_rays(torch.from_numpy(np.ascontiguousarray(o, np.float32)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda())
    assert all(x.is_cuda for x in out.values())
    assert out["t_hit"].dtype == torch.float32 and out["primitive_ids"].dtype == torch.int32
    return {k: out[k].cpu().numpy() for k in KEYS}


def _assert_same(got, want, what):
    for k in KEYS:
        diff = _bits(got[k]) != _bits(want[k])
        assert not diff.any(), (what, k, int(diff.sum()), np.argwhere(diff)[:5].tolist())


# ------------------------------------------------------------------------------------------------------------- meshes
def _mesh_one():
    return np.array([[0.1, 0.2, 0.3], [2.3, 0.4, 0.9], [0.7, 1.9, 1.4]], np.float32), np.array([[0, 1, 2]], np.int32)


def _mesh_quad():
    return (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32) * np.float32(4.0),
            np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def _mesh_sphere():
    vol, iso = mc.sphere_volume((24, 24, 24), 8.3)
    v, t, _ = mc.marching_cubes(vol, iso)
    return v, t


def _mesh_cases():
    """All 256 marching-cubes cases, non-manifold contacts included."""
    v, t, _ = mc.marching_cubes(*mc.case_volume())
    return v, t


def _mesh_soup():
    rng = np.random.default_rng(7)
    centre = rng.uniform(-3, 3, (257, 1, 3))
    v = (centre + rng.uniform(-0.6, 0.6, (257, 3, 3))).astype(np.float32).reshape(-1, 3)
    t = np.arange(257 * 3, dtype=np.int32).reshape(257, 3)
    t[10, 1] = t[10, 0]  # a few zero-area ones: a repeated vertex ...
    t[100] = t[100, 0]
    t[200, 2] = t[200, 1]
    v[3 * 50 + 1] = v[3 * 50]  # ... and equal coordinates under different indices
    return v, t


def _mesh_thin():
    """One thin triangle from corner to corner of the box (it lands in many cells) among small ones."""
    rng = np.random.default_rng(9)
    centre = rng.uniform(0.5, 9.5, (40, 1, 3))
    v = (centre + rng.uniform(-0.3, 0.3, (40, 3, 3))).astype(np.float32).reshape(-1, 3)
    v = np.concatenate([v, np.array([[0, 0, 0], [10, 10, 10], [10, 10.02, 9.99]], np.float32)])
    t = np.concatenate([np.arange(120, dtype=np.int32).reshape(40, 3), np.array([[120, 121, 122]], np.int32)])
    return v, t


MESHES = {"one_triangle": _mesh_one, "quad": _mesh_quad, "sphere": _mesh_sphere, "all_256_cases": _mesh_cases, "soup": _mesh_soup,
          "thin_across_the_box": _mesh_thin}


# ---------------------------------------------------------------------------------------------------------------- rays
def _ray_set(v, t, n_total):
    """At most about 4000 rays (n_total of them exactly): see the list in the module's tests."""
    from lidarnerf.raycast import default_grid_resolution
    rng = np.random.default_rng(len(v) * 31 + len(t))
    lo, hi = v.min(0), v.max(0)
    ext = np.maximum(hi - lo, np.float32(1e-3))
    inside = (lo + ext * np.array([0.47, 0.52, 0.55], np.float32)).astype(np.float32)
    O, D = [], []

    def add(o, d):
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        O.append(np.broadcast_to(o, d.shape).copy())
        D.append(d)

    fo, fd = rr.rays_at_features(v, t, inside)  # every vertex, edge midpoint, centroid (a subset on a large mesh), the six axes
    keep = np.arange(len(fo)) if len(fo) <= 1500 else np.concatenate([rng.choice(len(fo) - 6, 1494, replace=False), np.arange(len(fo) - 6, len(fo))])
    add(fo[keep], fd[keep])
    add(inside, rng.standard_normal((300, 3)))
    one, two = rng.standard_normal((120, 3)), rng.standard_normal((60, 3))  # one and two zero components
    one[np.arange(120), np.arange(120) % 3] = 0
    two[np.arange(60), np.arange(60) % 3] = 0
    two[np.arange(60), (np.arange(60) + 1) % 3] = 0
    add(rng.uniform(lo, hi, (120, 3)), one)
    add(rng.uniform(lo, hi, (60, 3)), two)
    outside = (lo - ext * 0.7 + rng.uniform(0, 1, (300, 3)) * ext * 2.4).astype(np.float32)  # origins around the box
    aim = rng.uniform(lo, hi, (300, 3)).astype(np.float32)
    add(outside[:200], aim[:200] - outside[:200])      # ... towards it
    add(outside[200:], outside[200:] - aim[200:])      # ... away from it
    add(outside[:60], rng.standard_normal((60, 3)))    # ... anywhere
    for grid in ((2, 3, 5), default_grid_resolution(len(t), np.concatenate([lo, hi])), PAST_ONE_TILE):
        _, w, planes = rr.grid_planes(lo, hi, grid)
        pick = lambda a, n: planes[a][rng.integers(0, len(planes[a]), n)]
        corner = np.stack([pick(0, 70), pick(1, 70), pick(2, 70)], 1)  # origins exactly ON boundary planes (all three)
        add(corner[:30], rng.standard_normal((30, 3)))
        add(corner[30:50], rr.AXES[rng.integers(0, 6, 20)])  # travelling along a cell edge
        in_plane = rng.standard_normal((20, 3))
        in_plane[np.arange(20), np.arange(20) % 3] = 0
        add(corner[50:], in_plane)  # travelling inside a boundary plane
        on_one = rng.uniform(lo, hi, (20, 3)).astype(np.float32)
        on_one[np.arange(20), np.arange(20) % 3] = corner[:20][np.arange(20), np.arange(20) % 3]
        add(on_one, rng.standard_normal((20, 3)))  # on one boundary plane
        start = rng.uniform(lo - ext * 0.3, hi + ext * 0.3, (40, 3)).astype(np.float32)
        add(start, corner[:40] - start)  # through cell corners
    bad_d = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], np.float32)
    add(inside, bad_d)
    bad_o = np.tile(inside, (2, 1))
    bad_o[0, 1], bad_o[1, 2] = np.nan, np.inf
    O.append(bad_o), D.append(np.array([[1, 0, 0], [0, 1, 0]], np.float32))
    add(inside + np.float32(1e7), rng.standard_normal((4, 3)))  # an origin the walk's arithmetic cannot resolve: all triangles
    add(inside, rng.standard_normal((4, 3)) * np.float32(1e-35))
    o, d = np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)
    assert len(o) <= n_total, len(o)
    extra = n_total - len(o)
    o = np.concatenate([o, np.broadcast_to(inside, (extra, 3))]).astype(np.float32)
    d = np.concatenate([d, rng.standard_normal((extra, 3)).astype(np.float32)])
    order = rng.permutation(n_total)  # the kinds mixed: every wave holds several
    return np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, triangles, rays_o, rays_d, restatement) of a mesh: computed once, shared, read-only."""
    v, t = MESHES[name]()
    o, d = _ray_set(v, t, RAY_COUNTS[-1] if name == "sphere" else 3000)
    want = rr.cast_rays(v, t, o, d)
    for a in (v, t, o, d) + tuple(want.values()):
        a.setflags(write=False)
    return v, t, o, d, want


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("name", list(MESHES))
def test_the_whole_output_equals_the_restatement_at_every_grid(name, grid):
    v, t, o, d, want = _case(name)
    hits = int((want["primitive_ids"] >= 0).sum())
    assert 0 < hits < len(o), "the ray set must both hit and miss"
    if grid == "past_one_scan_tile":
        assert np.prod(PAST_ONE_TILE) > _scan_tile() + 1000
    if grid == "one_scan_tile":
        assert np.prod(ONE_TILE) == _scan_tile()
    if grid == "one_past_a_scan_tile":
        assert np.prod(ONE_PAST_A_TILE) == _scan_tile() + 1
    scene = _scene(v, t, GRIDS[grid])
    got = _cast(scene, o, d)
    print(f"{name} / {grid}: grid {scene.grid}, {scene.entries} entries for {len(t)} triangles, {hits} of {len(o)} rays hit")
    _assert_same(got, want, (name, grid))
    assert scene.entries >= len(t) and (GRIDS[grid] is None or scene.grid == GRIDS[grid])
    if scene.grid == (1, 1, 1):
        assert scene.entries == len(t)


@pytest.mark.parametrize("n", RAY_COUNTS)
def test_ray_counts_around_a_wave_and_a_workgroup(n):
    v, t, o, d, want = _case("sphere")
    scene = _scene(v, t)
    got = _cast(scene, o[:n], d[:n])
    _assert_same(got, {k: want[k][:n] for k in KEYS}, n)
    empty = scene.cast_rays(torch.zeros((0, 6), device="cuda"))
    assert empty["t_hit"].shape == (0,) and empty["primitive_normals"].shape == (0, 3)


def test_two_builds_of_a_scene_give_identical_outputs():
    """The order of the entries inside a cell is arrival order (it may differ between the builds); no output may depend on it."""
    for name in ("all_256_cases", "thin_across_the_box"):
        v, t, o, d, want = _case(name)
        a, b = _scene(v, t, (6, 7, 3)), _scene(v, t, (6, 7, 3))
        assert a.entries == b.entries and torch.equal(a.cell_start, b.cell_start)
        sort = lambda s: [sorted(s.cell_tris[lo:hi].tolist()) for lo, hi in zip(s.cell_start[:-1].tolist(), s.cell_start[1:].tolist())]
        assert sort(a) == sort(b)  # the same lists as sets
        _assert_same(_cast(a, o, d), _cast(b, o, d), name)
        _assert_same(_cast(a, o, d), want, name)


def test_guard_words_behind_every_output_and_the_raw_entry_point():
    from lidarnerf import _hip
    v, t, o, d, want = _case("soup")
    s = _scene(v, t, (5, 4, 3))
    for n in (1, 65, 1000):
        ro, rd = torch.from_numpy(o[:n].copy()).cuda(), torch.from_numpy(d[:n].copy()).cuda()
        guard = 16
        bufs = {k: torch.full((n * w + guard,), SENTINEL, dtype=torch.int32, device="cuda")
                for k, w in (("t_hit", 1), ("primitive_ids", 1), ("primitive_normals", 3), ("incidences", 1))}
        for with_inc in (True, False):
            _hip.call("lnh_raycast_cast", s.vertices.data_ptr(), s.V, s.triangles.data_ptr(), s.T, s.box.data_ptr(), *s.grid,
                      s.cell_start.data_ptr(), s.cell_tris.data_ptr(), s.entries, ro.data_ptr(), rd.data_ptr(), n,
                      bufs["t_hit"].data_ptr(), bufs["primitive_ids"].data_ptr(), bufs["primitive_normals"].data_ptr(),
                      bufs["incidences"].data_ptr() if with_inc else None)
            torch.cuda.synchronize()
            for k, w in (("t_hit", 1), ("primitive_ids", 1), ("primitive_normals", 3), ("incidences", 1)):
                raw = bufs[k].cpu().numpy()
                assert (raw[n * w:] == SENTINEL).all(), ("guard words overwritten", k, n)
                assert np.array_equal(raw[:n * w].view(np.uint32), _bits(want[k][:n]).reshape(-1)), (k, n)
    # the workspace and the lists: guard words behind cell_start and cell_tris survive a rebuild through the C ABI
    L = _hip.lib()
    nx, ny, nz = s.grid
    cells = nx * ny * nz
    ws = torch.empty(int(L.lnh_raycast_workspace_size(s.V, s.T, nx, ny, nz, 0)), dtype=torch.uint8, device="cuda")
    cs = torch.full((cells + 1 + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    ct = torch.full((s.entries + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    _hip.call("lnh_raycast_build_count", s.vertices.data_ptr(), s.V, s.triangles.data_ptr(), s.T, s.box.data_ptr(), nx, ny, nz,
              ws.data_ptr(), ws.numel(), cs.data_ptr(), counts.data_ptr())
    assert counts.tolist()[2:] == [s.entries, 0]
    _hip.call("lnh_raycast_build_fill", s.vertices.data_ptr(), s.V, s.triangles.data_ptr(), s.T, s.box.data_ptr(), nx, ny, nz,
              ws.data_ptr(), ws.numel(), cs.data_ptr(), ct.data_ptr(), s.entries)
    torch.cuda.synchronize()
    assert (cs[cells + 1:] == SENTINEL).all() and (ct[s.entries:] == SENTINEL).all()
    assert torch.equal(cs[:cells + 1], s.cell_start) and int(ct[:s.entries].min()) >= 0 and int(ct[:s.entries].max()) < s.T
    assert sorted(ct[:s.entries].tolist()) == sorted(s.cell_tris.tolist())


def test_the_box_and_the_counts_of_the_bounds_pass():
    v, t, *_ = _case("sphere")
    s = _scene(v, t, 4)
    box = s.box.cpu().numpy()
    assert np.array_equal(_bits(box[:3]), _bits(v.min(0))) and np.array_equal(_bits(box[3:6]), _bits(v.max(0)))
    tri = v[t]
    assert np.array_equal(_bits(box[6:]), _bits((tri.max(1) - tri.min(1)).max(0)))
    assert s.bounds == (tuple(v.min(0).tolist()), tuple(v.max(0).tolist())) and s.counts.tolist()[:2] == [0, 0]


def test_unnormalised_directions_scale_t_and_leave_the_ids():
    v, t, o, d, want = _case("sphere")
    scene = _scene(v, t)
    with np.errstate(invalid="ignore"):
        big = np.abs(d[:1500]).max(1)
    plain = np.isfinite(d[:1500]).all(1) & (big > 1e-3) & (big < 1e3)  # (not the 1e-35 directions: scaled, they leave fp32's range)
    assert plain.sum() > 1400
    for scale in (np.float32(8.0), np.float32(1.0 / 1024)):  # powers of two: every operation scales exactly
        got = _cast(scene, o[:1500], d[:1500] * scale)
        assert np.array_equal(got["primitive_ids"][plain], want["primitive_ids"][:1500][plain])
        assert np.array_equal(_bits(got["t_hit"] * scale)[plain], _bits(want["t_hit"][:1500])[plain])
        assert np.array_equal(_bits(got["primitive_normals"])[plain], _bits(want["primitive_normals"][:1500])[plain])
        _assert_same(got, rr.cast_rays(v, t, o[:1500], d[:1500] * scale), scale)  # every ray: the restatement on the scaled rays
    got = _cast(scene, o[:1500], d[:1500] * np.float32(3.7))  # any scale: the restatement on the scaled rays
    _assert_same(got, rr.cast_rays(v, t, o[:1500], d[:1500] * np.float32(3.7)), "x 3.7")


def test_cast_captured_in_a_graph_equals_the_eager_call():
    v, t, o, d, want = _case("all_256_cases")
    scene = _scene(v, t)
    ro, rd = torch.from_numpy(o.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    eager = scene.cast_rays(ro, rd)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        scene.cast_rays(ro, rd)  # (warm-up on the side stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = scene.cast_rays(ro, rd)
    torch.cuda.current_stream().wait_stream(stream)
    for k in KEYS:
        captured[k].fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(captured[k].view(torch.int32), eager[k].view(torch.int32)), k
    _assert_same({k: captured[k].cpu().numpy() for k in KEYS}, want, "captured")
    # other rays in the same buffers: the replay reads them
    ro.copy_(torch.from_numpy(o[::-1].copy()).cuda()), rd.copy_(torch.from_numpy(d[::-1].copy()).cuda())
    graph.replay()
    torch.cuda.synchronize()
    _assert_same({k: captured[k].cpu().numpy() for k in KEYS}, {k: want[k][::-1] for k in KEYS}, "replayed on other rays")


def test_every_device_side_refusal_raises():
    from lidarnerf.raycast import RaycastingScene
    v, t = _mesh_quad()
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[2, 1] = bad
        with pytest.raises(ValueError, match="1 vertex coordinates are not finite"):
            RaycastingScene(w, t)
    for bad in (4, -1, 1 << 20):
        u = t.copy()
        u[1, 2] = bad
        with pytest.raises(ValueError, match=r"1 triangle indices are outside \[0, 4\)"):
            RaycastingScene(v, u)
    u = t.astype(np.int64)
    u[0, 0] = (1 << 32) + 1  # would wrap to a valid index in int32
    with pytest.raises(ValueError, match="1 triangle indices are outside"):
        RaycastingScene(v, torch.from_numpy(u).cuda())
    with pytest.raises(ValueError, match="empty mesh"):
        RaycastingScene(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    # the entry total: 2^19 triangles that each span the box, in 16^3 cells = 2^31 entries, one more than fit
    many = torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda").repeat(1 << 19, 1)
    with pytest.raises(ValueError, match=r"2147483648 entries.*coarser grid"):
        RaycastingScene(np.array([[0, 0, 0], [1, 1, 1], [1, 0, 1], [0, 1, 0]], np.float32), many, grid_resolution=16)
    assert RaycastingScene(np.array([[0, 0, 0], [1, 1, 1], [1, 0, 1]], np.float32), many[:1 << 10], grid_resolution=16).entries == 1 << 22
    # a build while a stream is capturing
    stream = torch.cuda.Stream()
    vd, td = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            with pytest.raises(RuntimeError, match="capturing"):
                RaycastingScene(vd, td)
    scene = RaycastingScene(vd, td)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.cast_rays(torch.zeros(3, 6))
    with pytest.raises(ValueError, match=r"\[N, 6\]"):
        scene.cast_rays(torch.zeros(3, 5, device="cuda"))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        scene.cast_rays(torch.zeros(3, 3, device="cuda"), torch.zeros(4, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.raydrop_features((2.0, 26.9), np.eye(4), 4, 8, intensities=torch.zeros(4, 8))
    with pytest.raises(ValueError, match="intensities"):
        scene.raydrop_features((2.0, 26.9), np.eye(4), 4, 8, intensities=torch.zeros(4, 7, device="cuda"))


# ------------------------------------------------------------------ the device's own marching-cubes output: a closed surface
SPHERE_CENTRE = np.array([(24 - 1) / 2 + 0.13 * (a + 1) for a in range(3)])


def test_closed_surface_properties_on_the_device_mesh(tmp_path):
    from lidarnerf.nerf import mesh
    from lidarnerf.raycast import RaycastingScene
    vol, iso = mc.sphere_volume((24, 24, 24), 8.3)
    dv, dt = mesh.marching_cubes(torch.from_numpy(vol).cuda(), float(iso))
    scene = RaycastingScene(dv, dt)
    assert scene.vertices.data_ptr() == dv.data_ptr()  # float32 / int32 GPU tensors are used as they are
    v, t = dv.cpu().numpy(), dt.cpu().numpy()
    o, d = rr.rays_at_features(v, t, np.array([11.37, 11.9, 12.21], np.float32))
    got = _cast(scene, o, d)
    assert (got["primitive_ids"] >= 0).all(), "a ray from inside escaped the closed surface"
    p = o.astype(np.float64) + d.astype(np.float64) * got["t_hit"].astype(np.float64)[:, None]
    assert np.abs(np.linalg.norm(p - SPHERE_CENTRE, axis=1) - 8.3).max() <= math.sqrt(3.0)
    rng = np.random.default_rng(1)
    unit = rng.standard_normal((2000, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    outside = (SPHERE_CENTRE + unit * rng.uniform(11, 30, (2000, 1))).astype(np.float32)
    away = _cast(scene, outside, outside - SPHERE_CENTRE.astype(np.float32))
    assert (away["primitive_ids"] == -1).all() and np.isinf(away["t_hit"]).all()
    towards = (SPHERE_CENTRE - outside.astype(np.float64)).astype(np.float32)
    near = _cast(scene, outside, towards)
    assert (near["primitive_ids"] >= 0).all()
    assert (near["t_hit"] < 1.0).all()  # t is in units of |d| = the distance to the centre: the near side
    depth = near["t_hit"].astype(np.float64) * np.linalg.norm(towards.astype(np.float64), axis=1)
    dist = np.linalg.norm(outside.astype(np.float64) - SPHERE_CENTRE, axis=1)
    assert (np.abs(dist - depth - 8.3) <= math.sqrt(3.0)).all()
    # the same scene from a file
    path = os.path.join(tmp_path, "sphere.ply")
    mesh.write_ply(path, v, t)
    _assert_same(_cast(RaycastingScene.from_ply(path, grid_resolution=5), o, d), got, "from_ply")


# -------------------------------------------------------------------------------------------------- hit dict and features
K = (2.0, 26.9)


def _pose():
    a, b = 0.3, -0.2
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = (rz @ rx).astype(np.float32)
    pose[:3, 3] = [11.4, 13.9, 12.2]
    return pose


@pytest.mark.parametrize("H,W", [(6, 16), (66, 1030)])
def test_hit_dict_and_raydrop_features_equal_their_torch_restatement(H, W):
    from lidarnerf import _hip
    from lidarnerf.dataset.rays import get_lidar_rays
    v, t, *_ = _case("sphere")
    scene, pose = _scene(v, t), _pose()
    dpose = torch.from_numpy(pose).cuda()
    ro, rd = torch.empty((H * W, 3), device="cuda"), torch.empty((H * W, 3), device="cuda")
    _hip.call("lnh_lidar_frame_rays", dpose.data_ptr(), 1, 0, H, W, K[0], K[1], ro.data_ptr(), rd.data_ptr())
    torch_rays = get_lidar_rays(dpose[None], K, H, W)  # the same convention (its trigonometry is torch's, not the kernel's)
    assert torch.allclose(torch_rays["rays_d"][0], rd, atol=1e-5) and torch.equal(torch_rays["rays_o"][0].contiguous(), ro)
    hit = scene.cast_rays(ro, rd)
    depths = hit["t_hit"]
    want = {"masks": depths != math.inf, "depths": depths, "normals": hit["primitive_normals"],
            "points": ro + rd / torch.linalg.norm(rd, dim=1, keepdim=True) * depths[:, None]}
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for got in (scene.intersect_rays(torch.cat([ro, rd], 1)), scene.intersect_rays(ro, rd),
                scene.intersect_lidar(np.asarray(K), pose, H, W), scene.intersect_lidar(K, dpose, H, W)):
        assert set(got) == {"masks", "depths", "points", "normals"} and all(x.is_cuda for x in got.values())
        assert got["masks"].dtype == torch.bool
        for k in want:
            assert same(got[k], want[k]), k
    n_hit = int(want["masks"].sum())
    assert n_hit == H * W  # the sensor sits inside the closed surface, off centre (misses: the quad below)
    assert bool(torch.isfinite(want["points"][want["masks"]]).all())
    inten = torch.rand(H, W, device="cuda")
    for intensities in (None, inten):
        img = scene.raydrop_features(K, pose, H, W, intensities=intensities)
        assert img.shape == (1, 10, H, W) and img.dtype == torch.float32 and img.is_cuda
        chan = lambda x: x.reshape(H, W)
        zeros = torch.zeros(H * W, device="cuda")
        rows = [want["masks"].float(), torch.where(want["masks"], depths, zeros), *hit["primitive_normals"].unbind(1),
                hit["incidences"], zeros if intensities is None else inten.reshape(-1), *rd.unbind(1)]
        for c, row in enumerate(rows):
            assert torch.equal(img[0, c].view(torch.int32), chan(row).contiguous().view(torch.int32)), c
        assert bool(torch.isfinite(img).all())


def test_the_frame_misses_where_there_is_no_mesh():
    v, t = _mesh_quad()
    scene, pose = _scene(v, t), np.eye(4, dtype=np.float32)
    pose[:3, 3] = [2, 2, 3]
    hit = scene.intersect_lidar((80.0, 160.0), pose, 8, 32)
    assert 0 < int(hit["masks"].sum()) < 8 * 32
    assert bool(torch.isinf(hit["depths"][~hit["masks"]]).all()) and not bool(hit["normals"][~hit["masks"]].any())
    img = scene.raydrop_features((80.0, 160.0), pose, 8, 32)
    assert torch.equal(img[0, 0].bool().reshape(-1), hit["masks"]) and not bool(img[0, 1].reshape(-1)[~hit["masks"]].any())


# ----------------------------------------------------------------------------------------------------------- the trainer
RENDER = dict(num_steps=768, upsample_steps=64)
MESH_R = 24


def _trainer(graph=False, rays=1024, **kw):
    """The small model and batches of tests/test_mesh_gpu.py's trainer tests."""
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph, render_kwargs=RENDER, **kw)
    assert tr.table is not None and tr.graph == graph
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, rays, 0, dev, (1, 1), "analytic") for s in range(8)]
    return tr, model, batches, poses


def _median_threshold(tr):
    from lidarnerf.nerf import mesh
    return float(mesh.density_volume(tr.model, MESH_R, fp16=tr.fp16).median())


def test_mesh_scene_is_the_mesh_save_mesh_writes(tmp_path):
    from lidarnerf.nerf import mesh
    tr, model, batches, poses = _trainer()
    torch.manual_seed(11)
    for s in range(4):
        tr.step(*batches[s])
    threshold = _median_threshold(tr)
    path = os.path.join(tmp_path, "scene.ply")
    n_v, n_t = tr.save_mesh(path, resolution=MESH_R, threshold=threshold)
    want_v, want_t = mesh.read_ply(path)
    was_training = model.training
    scene = tr.mesh_scene(resolution=MESH_R, threshold=threshold, grid_resolution=None)
    assert model.training == was_training and (scene.V, scene.T) == (n_v, n_t) and n_t > 0
    assert scene.vertices.is_cuda and scene.vertices.dtype == torch.float32 and scene.triangles.dtype == torch.int32
    assert np.array_equal(_bits(scene.vertices.cpu().numpy()), _bits(want_v)) and np.array_equal(scene.triangles.cpu().numpy(), want_t)
    box = model.aabb_infer.cpu().numpy()
    assert all(box[a] <= scene.bounds[0][a] and scene.bounds[1][a] <= box[3 + a] for a in range(3))
    hit = scene.intersect_lidar((2.0, 26.9), poses[0], 16, 64)
    assert int(hit["masks"].sum()) > 0 and bool(torch.isfinite(hit["depths"][hit["masks"]]).all())
    assert bool((hit["depths"][hit["masks"]] >= 0).all())
    img = scene.raydrop_features((2.0, 26.9), poses[0], 16, 64)
    assert img.shape == (1, 10, 16, 64) and bool(torch.isfinite(img).all())
    with pytest.raises(ValueError, match="empty mesh"):
        tr.mesh_scene(resolution=MESH_R, threshold=1e30)


def _train(graph, with_scene):
    tr, model, batches, poses = _trainer(graph=graph)
    torch.manual_seed(11)
    losses = []
    for s in range(20):
        losses.append(tr.step(*batches[s % 8]).detach().clone())
        if with_scene and s + 1 == 10:
            captured = (len(tr.capture_ms), len(tr._graphs)) if graph else None
            ptrs = (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version, tr.global_step)
            scene = tr.mesh_scene(resolution=MESH_R, threshold=_median_threshold(tr))
            assert scene.T > 0 and scene.intersect_lidar((2.0, 26.9), poses[0], 8, 32)["masks"].any()
            assert ptrs == (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version, tr.global_step)
    torch.cuda.synchronize()
    if graph:
        assert tr.graph and tr.graph_error is None
        if with_scene:
            assert captured == (len(tr.capture_ms), len(tr._graphs))  # nothing was captured again after the scene
    state = [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()]
    return state + [p.detach().clone() for p in tr.small] + [torch.stack(losses)]


@pytest.mark.parametrize("graph", [False, True])
def test_training_does_not_notice_a_mesh_scene(graph):
    """Twenty steps from one seed with a mesh_scene (and a cast) after the tenth against twenty without: table, fp16 copy, Adam
    moments, optimizer scalars, every MLP matrix and all losses bit for bit — launch by launch and as a captured step."""
    a = _train(graph, False)
    b = _train(graph, True)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), i
    assert torch.isfinite(a[-1]).all()
