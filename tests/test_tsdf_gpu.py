"""TSDF fusion on the device (csrc/tsdf.hip, lidarnerf/tsdf.py, MeshNVS.fit) against the NumPy restatement of its contracts
(tests/tsdf_ref.py).

Everything is compared BIT FOR BIT unless a test says otherwise: every operation of the header is one IEEE fp32 operation on both
sides (nothing is contracted: -ffp-contract=off; hipcc's fp32 division and square root are correctly rounded at the library's
flags), atan2 is taken in double and rounded on both sides, and the mesh filter is integer arithmetic.  Every raw call goes to
sentinel-filled outputs with guard words behind them and is made twice."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import tsdf_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = 0x5ca1ab1e
GUARD = 16
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _guarded(values, dtype):
    """A device buffer holding `values` with GUARD sentinel words behind them (all dtypes here are 4 bytes wide, or bytes)."""
    flat = torch.from_numpy(np.array(values).reshape(-1)).cuda()
    assert flat.dtype == dtype
    if dtype == torch.uint8:
        guard = torch.full((GUARD,), 0xa5, dtype=torch.uint8, device="cuda")
    else:
        guard = torch.full((GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(dtype)
    return torch.cat([flat, guard])


def _guard_ok(buf, n):
    tail = buf[n:]
    want = 0xa5 if buf.dtype == torch.uint8 else SENTINEL
    return bool(((tail if buf.dtype == torch.uint8 else tail.view(torch.int32)) == want).all())


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _integrate_raw(panos, w2l, K, max_depth, lo, step, dims, trunc, sum0, count0):
    """lnh_tsdf_integrate through the C ABI, twice from the same earlier content; (sum, count) as NumPy."""
    from lidarnerf import _hip
    n = dims[0] * dims[1] * dims[2]
    d_panos, d_w2l = torch.from_numpy(np.array(panos, dtype=F)).cuda(), torch.from_numpy(np.array(w2l, dtype=F)).cuda()
    Fr, H, W = panos.shape
    out = []
    for _ in range(2):
        s = _guarded(np.asarray(sum0, F), torch.float32)
        c = _guarded(np.asarray(count0, np.uint32).view(np.int32), torch.int32)
        _hip.call("lnh_tsdf_integrate", d_panos.data_ptr(), d_w2l.data_ptr(), Fr, H, W, float(K[0]), float(K[1]), float(max_depth),
                  _f3(lo), _f3(step), *dims, float(trunc), s.data_ptr(), c.data_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(s, n) and _guard_ok(c, n), "guard words overwritten"
        out.append((s[:n].cpu().numpy().reshape(dims), c[:n].cpu().numpy().view(np.uint32).reshape(dims)))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])
    return out[0]


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _matrices(kind, n, rng):
    """n world -> lidar matrices [n,12] float32: identity, translated, or rotated and translated."""
    out = []
    for k in range(n):
        R = _rotation(rng.standard_normal(3), rng.uniform(0.2, 2.5)) if kind == "rotated" else np.eye(3)
        t = np.zeros(3) if kind == "identity" else rng.uniform(-0.6, 0.6, 3)
        out.append(np.concatenate([R, t[:, None]], 1).reshape(12))
    return np.asarray(out, F)


def _panos(Fr, H, W, rng, lo=1.0, hi=5.0, special=True):
    p = rng.uniform(lo, hi, (Fr, H, W)).astype(F)
    if special:
        for value in (0.0, -1.0, np.nan, np.inf, -np.inf):
            p[rng.random(p.shape) < 0.04] = value
    return p


CASES = {
    # name: dims, frames, image, matrices, K, lattice lo, step, trunc
    "2x2x2_identity": ((2, 2, 2), 1, (4, 8), "identity", (30.0, 60.0), (-1.0, -1.1, -0.4), (2.0, 2.0, 1.0), 1.5),
    "3x5x67_translated": ((3, 5, 67), 2, (6, 16), "translated", (30.0, 60.0), (-2.0, -2.0, -2.0), (2.0, 1.0, 0.06), 0.7),
    "17x9x130_rotated": ((17, 9, 130), 5, (6, 16), "rotated", (40.0, 80.0), (-3.0, -2.0, -3.0), (0.4, 0.5, 0.05), 0.9),
    "33x31x29_rotated_big_image": ((33, 31, 29), 5, (66, 1030), "rotated", (2.0, 26.9), (-4.0, -4.0, -2.0), (0.25, 0.27, 0.15), 0.75),
    "33x31x29_one_frame": ((33, 31, 29), 1, (4, 8), "rotated", (45.0, 90.0), (-4.0, -4.0, -2.0), (0.25, 0.27, 0.15), 0.75),
    # more than 65535 bricks along y, and more than 65535 workgroups along z: the workgroup index is decomposed, not a 3-D grid
    "2x262148x3_long_y": ((2, 262148, 3), 1, (4, 8), "rotated", (45.0, 90.0), (-1.0, -4.0, -1.0), (2.0, 3e-5, 1.0), 0.75),
    "2x2x1048580_long_z": ((2, 2, 1048580), 1, (4, 8), "rotated", (45.0, 90.0), (-1.0, -1.0, -4.0), (2.0, 2.0, 8e-6), 0.75),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    dims, Fr, (H, W), kind, K, lo, step, trunc = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    panos, w2l = _panos(Fr, H, W, rng), _matrices(kind, Fr, rng)
    sum0 = rng.standard_normal(dims).astype(F)  # the accumulators hold earlier content on entry
    count0 = rng.integers(0, 7, dims).astype(np.uint32)
    want = ref.integrate(panos, w2l, *K, 6.0, F(lo), F(step), dims, F(trunc), sum0, count0)
    for a in (panos, w2l, sum0, count0, *want):
        a.setflags(write=False)
    return panos, w2l, K, 6.0, F(lo), F(step), dims, F(trunc), sum0, count0, want


@pytest.mark.parametrize("name", list(CASES))
def test_integrate_matches_the_restatement_bit_for_bit(name):
    *args, (want_s, want_c) = _case(name)
    count0, Fr = args[9], len(args[0])
    seen = want_c - count0
    print(f"{name}: {seen.sum()} observations of {seen.size * Fr} point-frames, {int((seen == 0).sum())} points unobserved")
    assert seen.sum() > 0 and (seen.max() == Fr or Fr == 5)
    if name != "2x2x2_identity":
        assert (seen == 0).any()
    got_s, got_c = _integrate_raw(*args)
    assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:5]
    diff = _bits(got_s) != _bits(want_s)
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5])


@pytest.mark.parametrize("name", ["17x9x130_rotated", "33x31x29_rotated_big_image"])
def test_two_plus_three_frames_are_five(name):
    panos, w2l, K, md, lo, step, dims, trunc, sum0, count0, (want_s, want_c) = _case(name)
    s2, c2 = _integrate_raw(panos[:2], w2l[:2], K, md, lo, step, dims, trunc, sum0, count0)
    s5, c5 = _integrate_raw(panos[2:], w2l[2:], K, md, lo, step, dims, trunc, s2, c2)
    assert np.array_equal(_bits(s5), _bits(want_s)) and np.array_equal(c5, want_c)


def test_integrate_special_lattice_points():
    """Lattice points on the sensor (r = 0), beyond max_depth, above and below the image rows, and on the column seam behind the
    sensor on both sides of the wrap."""
    H, W, K, md = 4, 8, (30.0, 60.0), 5.0
    dims, lo, step = (4, 5, 5), F([-3.0, -0.2, -4.0]), F([1.0, 0.1, 2.0])  # x -3..0, y -0.2..0.2, z -4..4
    panos = np.full((2, H, W), 5.0, F)
    panos[1, :, 0] = 2.0  # the seam column of the second frame is nearer
    w2l = _matrices("identity", 2, None)
    zeros = np.zeros(dims, F), np.zeros(dims, np.uint32)
    want_s, want_c = ref.integrate(panos, w2l, *K, md, lo, step, dims, F(0.6), *zeros)
    no_wrap = ref.integrate(panos, w2l, *K, md, lo, step, dims, F(0.6), *zeros, wrap=False)[1]
    px, py, pz = ref.lattice_axes(lo, step, dims)
    r = np.sqrt((px * px + py * py) + pz * pz)
    assert (r == 0).sum() == 1 and want_c[r == 0] == 0                      # on the sensor
    assert (r >= md).any() and (want_c[r >= md] == 0).all()                 # beyond max_depth
    assert (want_c[:, :, 0] == 0).all() and (want_c[:, :, 4] == 0).all()    # z = -4, 4: below and above the rows
    assert (want_c[:3, :2, 2] > 0).all() and (no_wrap[:3, :2, 2] == 0).all()  # the seam: observed only through the wrap
    assert (want_c[:3, 3:, 2] > 0).all() and np.array_equal(no_wrap[:3, 3:, 2], want_c[:3, 3:, 2])
    got_s, got_c = _integrate_raw(panos, w2l, K, md, lo, step, dims, 0.6, *zeros)
    assert np.array_equal(got_c, want_c) and np.array_equal(_bits(got_s), _bits(want_s))


# ------------------------------------------------------------------------------------------------------------ finalize
def _finalize_raw(s, c, min_count):
    from lidarnerf import _hip
    dims, n = s.shape, s.size
    ds, dc = torch.from_numpy(np.array(s)).cuda(), torch.from_numpy(np.array(c).view(np.int32)).cuda()
    out = []
    for _ in range(2):
        vol = _guarded(np.full(n, np.nan, F), torch.float32)
        _hip.call("lnh_tsdf_finalize", ds.data_ptr(), dc.data_ptr(), *dims, int(min_count), vol.data_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(vol, n)
        out.append(vol[:n].cpu().numpy().reshape(dims))
    assert np.array_equal(_bits(out[0]), _bits(out[1]))
    return out[0]


def test_finalize():
    *_, (s, c) = _case("17x9x130_rotated")
    for min_count in (1, 2, 7):
        want = ref.finalize(s, c, min_count)
        assert (want == ref.FILL).any() and (want != ref.FILL).any()
        assert np.array_equal(_bits(_finalize_raw(s, c, min_count)), _bits(want))
    assert not np.array_equal(ref.finalize(s, c, 1), ref.finalize(s, c, 2))
    nothing = _finalize_raw(s, np.zeros_like(c), 1)  # an all-unobserved lattice: the fill everywhere, no division by 0 shows
    assert (nothing == ref.FILL).all()
    from lidarnerf.nerf import mesh
    v, t = mesh.marching_cubes(torch.from_numpy(nothing).cuda(), 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ vertex mask and filter
def _observed_raw(vertices, count, min_count):
    from lidarnerf import _hip
    V = len(vertices)
    dv = torch.from_numpy(np.array(vertices, dtype=F)).cuda()
    dc = torch.from_numpy(np.array(count, dtype=np.uint32).view(np.int32)).cuda()
    out = []
    for _ in range(2):
        keep = _guarded(np.full(V, 7, np.uint8), torch.uint8)
        _hip.call("lnh_mesh_vertex_observed", dv.data_ptr(), V, dc.data_ptr(), *count.shape, int(min_count), keep.data_ptr())
        torch.cuda.synchronize()
        assert _guard_ok(keep, V)
        out.append(keep[:V].cpu().numpy())
    assert np.array_equal(out[0], out[1])
    return out[0]


def test_vertex_mask():
    count = np.zeros((3, 3, 3), np.uint32)
    count[0, 0, 0] = count[1, 0, 0] = count[1, 1, 0] = 2
    v = F([[0.5, 0, 0], [1, 0.5, 0], [1, 0, 0.5], [1, 0, 0], [2, 2, 2], [1.5, 0, 0], [-0.5, 0, 0], [np.nan, 0, 0], [0, 0, 2.5],
           [0, 0, 0], [1, 1, 0], [0.5, 0.5, 0], [2, 0, 0]])  # on edges, ON lattice points, outside, NaN, inside a face
    for min_count in (1, 2, 3):
        want = ref.vertex_observed(v, count, min_count)
        assert np.array_equal(_observed_raw(v, count, min_count), want)
    assert ref.vertex_observed(v, count, 1).tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    # the room's own marching-cubes vertices: 7242 of them, 29 workgroups
    room, (_, _, parts) = ref.room(), ref.room_mesh()
    got = _observed_raw(parts["vertices"], room["count"], 1)
    assert np.array_equal(got, parts["keep"]) and 0 < got.sum() < len(got)


def _filter_raw(vertices, keep, triangles, max_v=None, max_t=None):
    """count + emit through the C ABI with guard words; capacities default to the counts."""
    from lidarnerf import _hip
    L = _hip.lib()
    V, T = len(vertices), len(triangles)
    dv, dk = torch.from_numpy(np.array(vertices, dtype=F)).cuda(), torch.from_numpy(np.array(keep, dtype=np.uint8)).cuda()
    dt = torch.from_numpy(np.array(triangles, dtype=np.int32)).cuda()
    need = int(L.lnh_mesh_filter_workspace_size(V, T))
    assert need > 0
    out = []
    for _ in range(2):
        ws = _guarded(np.full(need, 0xcd, np.uint8), torch.uint8)
        counts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        _hip.call("lnh_mesh_filter_count", dk.data_ptr(), V, dt.data_ptr(), T, ws.data_ptr(), need, counts.data_ptr())
        Vk, Tk, z0, z1 = counts.tolist()
        assert z0 == 0 and z1 == 0
        cap_v, cap_t = (Vk if max_v is None else max_v), (Tk if max_t is None else max_t)
        ov = _guarded(np.full(cap_v * 3, SENTINEL, np.int32), torch.int32)
        ot = _guarded(np.full(cap_t * 3, SENTINEL, np.int32), torch.int32)
        if cap_v:
            _hip.call("lnh_mesh_filter_emit", dv.data_ptr(), dk.data_ptr(), V, dt.data_ptr(), T, ws.data_ptr(), need, ov.data_ptr(),
                      cap_v, ot.data_ptr(), cap_t)
        torch.cuda.synchronize()
        assert _guard_ok(ws, need) and _guard_ok(ov, cap_v * 3) and _guard_ok(ot, cap_t * 3), "guard words overwritten"
        out.append(((Vk, Tk), ov[:cap_v * 3].cpu().numpy().view(np.float32).reshape(-1, 3), ot[:cap_t * 3].cpu().numpy().reshape(-1, 3)))
    assert out[0][0] == out[1][0] and np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and np.array_equal(out[0][2], out[1][2])
    return out[0]


def _random_mesh(V, T, seed, keep_share=0.8):
    rng = np.random.default_rng(seed)
    vertices = rng.standard_normal((V, 3)).astype(F)
    triangles = rng.integers(0, V, (T, 3)).astype(np.int32)
    triangles[rng.integers(0, T, 5)] = [-1, 0, V - 1]   # indices outside [0, V): such a triangle goes
    triangles[rng.integers(0, T, 5), 1] = V
    keep = (rng.random(V) < keep_share).astype(np.uint8)
    return vertices, keep, triangles


# csrc/tsdf.hip: 256 indices per workgroup; k_mf_scan scans the workgroup totals in tiles of 4096 (csrc/scan.h), so more than
# 4096 * 256 = 1 048 576 vertices or triangles need a second tile
# totals: 4095, 4096 and 4097 of them sit on both sides of the tile's end (V, T = 1 048 320, 1 048 576, 1 048 577)
@pytest.mark.parametrize("V,T", [(1, 1), (255, 300), (4095, 4097), (4096, 4096), (4097, 4095), (20000, 41234), (1048320, 1048577),
                                 (1048576, 1048576), (1048577, 1048320), (1100000, 1200000)])
def test_filter_matches_the_restatement(V, T):
    vertices, keep, triangles = _random_mesh(V, T, V + T)
    if V == 1:
        keep[:], triangles[:] = 1, 0
    want_v, want_t = ref.mesh_filter(vertices, keep, triangles)
    (Vk, Tk), got_v, got_t = _filter_raw(vertices, keep, triangles)
    assert (Vk, Tk) == (len(want_v), len(want_t)) and Vk > 0 and Tk > 0
    assert np.array_equal(_bits(got_v), _bits(want_v)) and np.array_equal(got_t, want_t)
    # references only kept vertices, and keeps the triangle order: mapped back, the result is a subsequence of the input
    assert got_t.min() >= 0 and got_t.max() < Vk
    old = np.flatnonzero(keep)[got_t]
    stays = ((triangles >= 0) & (triangles < V)).all(1)
    stays &= keep[np.clip(triangles, 0, V - 1)].all(1).astype(bool)
    assert np.array_equal(old, triangles[stays])


def test_filter_masks_of_all_ones_and_all_zeros_and_short_capacities():
    from lidarnerf import tsdf
    _, _, parts = ref.room_mesh()
    v, t, keep = parts["vertices"], parts["triangles"], parts["keep"]
    (Vk, Tk), got_v, got_t = _filter_raw(v, np.ones(len(v), np.uint8), t)
    assert (Vk, Tk) == (len(v), len(t)) and np.array_equal(_bits(got_v), _bits(v)) and np.array_equal(got_t, t)
    (Vk, Tk), got_v, got_t = _filter_raw(v, np.zeros(len(v), np.uint8), t)  # counts 0, 0: no emit (capacity 0 is refused)
    assert (Vk, Tk) == (0, 0) and got_v.shape == (0, 3) and got_t.shape == (0, 3)
    dv, dt = torch.from_numpy(v.copy()).cuda(), torch.from_numpy(t.copy()).cuda()
    ev, et = tsdf.filter_mesh(dv, dt, torch.zeros(len(v), dtype=torch.uint8, device="cuda"))
    assert ev.shape == (0, 3) and et.shape == (0, 3) and ev.is_cuda and et.dtype == torch.int32
    # the room's own mask, with capacities one short, then of one row: a prefix, and the guard words stay (_filter_raw asserts)
    want_v, want_t = ref.mesh_filter(v, keep, t)
    (Vk, Tk), got_v, got_t = _filter_raw(v, keep, t, max_v=len(want_v) - 1, max_t=len(want_t) - 1)
    assert (Vk, Tk) == (len(want_v), len(want_t))
    assert np.array_equal(_bits(got_v), _bits(want_v[:-1])) and np.array_equal(got_t, want_t[:-1])
    (Vk, Tk), got_v, got_t = _filter_raw(v, keep, t, max_v=1, max_t=1)
    assert np.array_equal(_bits(got_v), _bits(want_v[:1])) and np.array_equal(got_t, want_t[:1])
    # a vertex mask that removes every triangle but not every vertex: the vertices alone
    lone = np.zeros(len(v), np.uint8)
    lone[t[0, 0]] = 1
    pv, pt = tsdf.filter_mesh(dv, dt, torch.from_numpy(lone).cuda())
    assert pv.shape == (1, 3) and pt.shape == (0, 3) and np.array_equal(_bits(pv.cpu().numpy()), _bits(v[t[0, 0]][None]))
    pv, pt = tsdf.filter_mesh(dv, dt, torch.from_numpy(keep.copy()).cuda())
    assert np.array_equal(_bits(pv.cpu().numpy()), _bits(want_v)) and np.array_equal(pt.cpu().numpy(), want_t)


# ------------------------------------------------------------------------------------------------------ the Python layer
ROOM_BOX = (ref.ROOM_LO - 0.55, ref.ROOM_HI + 0.55)


def test_extract_mesh_equals_the_hand_chained_restatement_on_the_room():
    from lidarnerf import nvs, tsdf
    from lidarnerf.raycast import RaycastingScene
    room = ref.room()
    vol = tsdf.TSDFVolume(ROOM_BOX, voxel_size=ref.ROOM_H)
    assert vol.dims == (66, 46, 29) and np.array_equal(vol.lo, room["lo"]) and np.array_equal(vol.step, room["step"])
    assert vol.truncation == float(room["trunc"])
    poses = torch.from_numpy(room["poses"].copy()).cuda()
    w2l = torch.stack([nvs.inverse_pose(p)[:3].reshape(12) for p in poses]).cpu().numpy()
    assert np.array_equal(w2l, room["w2l"])  # the kernel and the restatement see the same numbers
    vol.integrate(room["panos"][:1], room["poses"][:1], ref.ROOM_K)  # NumPy in, any number of calls
    vol.integrate(torch.from_numpy(room["panos"][1:].copy()).cuda(), poses[1:], ref.ROOM_K)
    assert vol.frames == 4
    assert np.array_equal(vol.count.cpu().numpy().view(np.uint32), room["count"])
    assert np.array_equal(_bits(vol.sum.cpu().numpy()), _bits(room["sum"]))
    want_v, want_t, parts = ref.room_mesh()
    assert np.array_equal(_bits(vol.volume().cpu().numpy()), _bits(parts["volume"]))
    assert np.array_equal(_bits(vol.volume(2).cpu().numpy()), _bits(ref.finalize(room["sum"], room["count"], 2)))
    v, t = vol.extract_mesh()
    assert v.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    assert np.array_equal(t.cpu().numpy(), want_t)
    diff = _bits(v.cpu().numpy()) != _bits(want_v)
    assert not diff.any(), int(diff.sum())
    scene = vol.scene()
    assert isinstance(scene, RaycastingScene) and scene.T == len(want_t) and scene.V == len(want_v)
    empty = tsdf.TSDFVolume(ROOM_BOX, resolution=8)
    with pytest.raises(RuntimeError, match="no surface"):
        empty.extract_mesh()
    with pytest.raises(RuntimeError, match="no surface"):
        empty.scene()
    with pytest.raises(ValueError, match="panos"):
        vol.integrate(room["panos"], room["poses"][:2], ref.ROOM_K)


def test_sphere_bound_on_the_device():
    """The bound of tests/test_tsdf_cpu.py::test_sphere_vertices_lie_on_the_sphere (interpolation h^2 / (8 (d0 - h)) plus the rounding
    term derived there), on TSDFVolume.extract_mesh."""
    from lidarnerf import tsdf
    S = ref.SPHERE
    vol = tsdf.TSDFVolume(([S["box"][0]] * 3, [S["box"][1]] * 3), voxel_size=S["h"])
    assert vol.dims == (41, 41, 41)
    vol.integrate(np.full(S["HW"], S["d0"], F), np.eye(4, dtype=F), S["K"])
    v, t = vol.extract_mesh()
    err, bound, excess, allowed = ref.check_sphere_vertices(v.cpu().numpy())
    print(f"sphere on the device: {len(v)} vertices, max |r - d0| {err:.3e} (bound {bound:.3e}); elevation excess {excess:.3f} "
          f"pixels (allowed {allowed:.3f})")
    assert len(v) > 500 and err <= bound and allowed == 0.5 and excess <= allowed


def _room_frames(H=None, W=None, sensors=ref.ROOM_SENSORS):
    """Frame dicts of the room with the keys of extract_dataset_frame that fit reads; intensity = a smooth function of height."""
    H, W = ref.ROOM_HW if H is None else (H, W)
    frames = []
    for s in sensors:
        pano = ref.room()["panos"][ref.ROOM_SENSORS.index(s)] if (H, W) == ref.ROOM_HW else ref.room_depths(s, H, W, *ref.ROOM_K)
        z = pano * ref.pixel_directions(H, W, *ref.ROOM_K)[..., 2].astype(F) + F(s[2])
        frames.append({"pano": pano, "intensities": (0.5 + 0.1 * z).astype(F), "lidar_pose": ref.translation_pose(s),
                       "lidar_K": ref.ROOM_K, "lidar_H": H, "lidar_W": W})
    return frames


@functools.lru_cache(maxsize=None)
def _fitted():
    from lidarnerf.nvs import MeshNVS
    return MeshNVS.fit(_room_frames(), voxel_size=ref.ROOM_H, box=ROOM_BOX)


def test_fit_on_the_room_closes_the_loop_through_predict_frame():
    """The closed-loop conditions of the issue through MeshNVS.predict_frame at two training poses."""
    from lidarnerf.nvs import MeshNVS
    model = _fitted()
    assert isinstance(model, MeshNVS) and model.volume.dims == (66, 46, 29) and model.volume.frames == 4
    want_v, want_t, _ = ref.room_mesh()
    assert np.array_equal(_bits(model.scene.vertices.cpu().numpy()), _bits(want_v))
    assert np.array_equal(model.scene.triangles.cpu().numpy(), want_t)
    n_cloud = sum(int((f["pano"] > 0).sum()) for f in _room_frames())
    assert model.points.shape == (n_cloud, 3) and model.point_intensities.shape == (n_cloud,)
    H, W = ref.ROOM_HW
    for frame in (0, 1):
        pick, o, d, depth = ref.closed_loop_rays(frame)
        out = model.predict_frame(ref.ROOM_K, ref.translation_pose(ref.ROOM_SENSORS[frame]), H, W, compact=False)
        pano = out["pano"].cpu().numpy().reshape(-1)[pick].astype(np.float64)
        normals = out["hit_dict"]["normals"].cpu().numpy()[pick]
        share, err, facing = ref.closed_loop_figures(np.where(pano > 0, pano, np.inf), normals, d, depth)
        print(f"fit, frame {frame}: hit share {share:.3f}, median {np.median(err):.4f} h, 95th percentile "
              f"{np.percentile(err, 95):.4f} h, max {err.max():.3f} h, normals facing {facing}")
        assert share >= 0.85 and np.median(err) <= 0.1 and np.percentile(err, 95) <= 0.5 and facing
        inten = out["intensities"].cpu().numpy().reshape(-1)[pick][pano > 0]
        assert np.isfinite(inten).all() and inten.min() > 0.2 and inten.max() < 0.9  # the k-NN index holds the cloud


def test_fit_defaults_and_mixed_frame_sizes():
    """No box given: the cloud's bounds plus the margin.  Frames of two sizes are integrated call by call."""
    from lidarnerf.nvs import MeshNVS
    frames = _room_frames(16, 64, ref.ROOM_SENSORS[:2]) + _room_frames(32, 48, ref.ROOM_SENSORS[2:])
    frames[0]["pano"] = np.where(np.random.default_rng(0).random((16, 64)) < 0.1, F(-1), frames[0]["pano"]).astype(F)  # NeRF-MVL's -1
    model = MeshNVS.fit(frames, voxel_size=0.4, intensity_interpolate_k=3)
    assert model.volume.frames == 4 and model.k == 3
    lo, hi = model.points.min(0).values.cpu().numpy(), model.points.max(0).values.cpu().numpy()
    assert np.allclose(model.volume.lo, lo - 1.6, atol=1e-5) and (lo > ref.ROOM_LO - 1e-3).all() and (hi < ref.ROOM_HI + 1e-3).all()
    assert model.points.shape[0] == sum(int((f["pano"] > 0).sum()) for f in frames)
    assert model.scene.T > 100
    coarse = MeshNVS.fit(frames, resolution=24)
    assert coarse.volume.dims == (24, 24, 24) and coarse.scene.T > 50


def test_raydrop_dataset_feeds_the_unet_trainer():
    import unet_ref
    from lidarnerf.unet import RayDropUNet
    from lidarnerf.unet_trainer import RayDropUNetTrainer
    model = _fitted()
    frames = _room_frames(32, 48, ref.ROOM_SENSORS[:2])
    frames[1]["pano"] = np.where(np.random.default_rng(1).random((32, 48)) < 0.2, F(0), frames[1]["pano"]).astype(F)
    images, masks = model.raydrop_dataset(frames)
    assert images.shape == (2, 10, 32, 48) and masks.shape == (2, 32, 48) and images.is_cuda and masks.dtype == torch.float32
    assert images.is_contiguous()
    for k, f in enumerate(frames):
        want = model.raydrop_features(f["lidar_K"], f["lidar_pose"], 32, 48)  # channel order: raydrop_features'
        assert torch.equal(images[k].view(torch.int32), want[0].contiguous().view(torch.int32))
        assert np.array_equal(masks[k].cpu().numpy(), (f["pano"] != 0).astype(F))
    assert 0 < float(masks[1].mean()) < 1 and float(images[:, 0].mean()) > 0.5  # most rays hit the mesh
    net = RayDropUNet()
    net.load_state_dict(unet_ref.hash_state_dict())
    trainer = RayDropUNetTrainer(net.cuda(), lr=1e-4)
    loss = trainer.train_step(images, masks)
    assert loss.dim() == 0 and math.isfinite(float(loss))
    out = model.predict_frame_with_raydrop(ref.ROOM_K, frames[0]["lidar_pose"], 32, 48, model=net)
    assert out["pano"].shape == (32, 48) and bool(torch.isfinite(out["pano"]).all())


def test_training_does_not_notice_a_fit():
    """Six steps of an unrelated LidarTrainer from one seed with a MeshNVS.fit after the third against six without: table, Adam
    moments, optimizer scalars, every MLP matrix and all losses bit for bit."""
    import test_mesh_gpu as M
    from lidarnerf.nvs import MeshNVS
    frames = _room_frames(16, 64, ref.ROOM_SENSORS[:2])

    def run(with_fit):
        tr, model, batches = M._trainer()
        torch.manual_seed(11)
        losses = []
        for s in range(6):
            losses.append(tr.step(*batches[s]).detach().clone())
            if with_fit and s == 2:
                assert MeshNVS.fit(frames, voxel_size=0.5).scene.T > 0
        torch.cuda.synchronize()
        state = [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()]
        return state + [p.detach().clone() for p in tr.small] + [torch.stack(losses)]

    a, b = run(False), run(True)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), i
    assert torch.isfinite(a[-1]).all()
