"""TSDF fusion without a GPU: the entry points of csrc/tsdf.hip exported, declared and bound; every refusal before any launch;
the NumPy restatement (tests/tsdf_ref.py) against what the method must do — frames split over calls, the column wrap, dropped
frames, a sphere of constant depth held to its interpolation bound, and the closed loop of the box room (fuse, mesh, cast
back) on the restatement together with tests/marching_cubes_ref.py and tests/raycast_ref.py; the Python surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import raycast_ref as rc
import tsdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2  # LNH_ERR_INVALID_ARG, LNH_ERR_UNSUPPORTED (include/lidarnerf_hip.h)
NAMES = ("lnh_tsdf_integrate", "lnh_tsdf_finalize", "lnh_mesh_vertex_observed", "lnh_mesh_filter_workspace_size",
         "lnh_mesh_filter_count", "lnh_mesh_filter_emit")
F = np.float32


# -------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_declared_and_bound():
    from lidarnerf import _hip
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    L = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(L, name), name
        assert re.search(r"LNH_API (int|uint64_t|void) " + name + r"\(", text), name
    P, U32, U64, F32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    want = {"lnh_tsdf_integrate": [P, P, U32, U32, U32, F32, F32, F32, P, P, U32, U32, U32, F32, P, P],
            "lnh_tsdf_finalize": [P, P, U32, U32, U32, U32, P],
            "lnh_mesh_vertex_observed": [P, U32, P, U32, U32, U32, U32, P],
            "lnh_mesh_filter_count": [P, U32, P, U32, P, U64, P],
            "lnh_mesh_filter_emit": [P, P, U32, P, U32, P, U64, P, U32, P, U32]}
    for name, sig in want.items():
        assert _hip._SIGS[name] == sig and getattr(L, name).argtypes == sig + [P], name  # the stream comes last
        assert _hip._OPTIONAL[name] == "TSDF fusion"
    assert L.lnh_mesh_filter_workspace_size.restype is U64 and L.lnh_mesh_filter_workspace_size.argtypes == [U32, U32]
    # the header states the argument lists the binding uses
    flat = re.sub(r"\s+", " ", text)
    assert ("lnh_tsdf_integrate(const float *panos, const float *world_to_lidar, uint32_t F, uint32_t H, uint32_t W, float fov_up, "
            "float fov, float max_depth, const float *lo, const float *step, uint32_t nx, uint32_t ny, uint32_t nz, float trunc, "
            "float *sum, uint32_t *count, lnh_stream_t stream)") in flat
    assert ("lnh_mesh_filter_emit(const float *vertices, const uint8_t *keep, uint32_t V, const int32_t *triangles, uint32_t T, "
            "void *ws, uint64_t ws_bytes, float *out_vertices, uint32_t max_vertices, int32_t *out_triangles, "
            "uint32_t max_triangles, lnh_stream_t stream)") in flat
    assert "sum += min(s / trunc, 1); count += 1" in text and "a column that rounds to W is column 0" in text


def test_the_projection_has_one_copy():
    """pano_pixel's arithmetic lives in csrc/pano_geom.h; convert.hip and tsdf.hip both call it."""
    csrc = os.path.join(ROOT, "lidar-nerf_amd", "csrc")
    geom, conv, tsdf = (open(os.path.join(csrc, n)).read() for n in ("pano_geom.h", "convert.hip", "tsdf.hip"))
    assert geom.count("uint32_t pano_pixel_xyz(") == 1
    for text in (conv, tsdf):
        assert '#include "pano_geom.h"' in text and "atan2(" not in text  # (no projection of its own)
    assert "pano_pixel_xyz<false>" in conv and "pano_pixel_xyz<true>" in tsdf


def test_workspace_size():
    from lidarnerf import _hip
    size = _hip.lib().lnh_mesh_filter_workspace_size
    assert size(1, 1) >= 4 * 5 and size(1, 1) % 16 == 0
    assert size(4096, 8000) >= 4 * 4096 + 8 * (16 + 32)
    assert size(1000001, 1) > size(1000000, 1) - 16 and size((1 << 31) - 1, (1 << 31) - 1) > 0
    for V, T in ((0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31), (0xffffffff, 0xffffffff)):
        assert size(V, T) == 0, (V, T)


def test_every_refusal_comes_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced or a kernel is launched
    f3 = lambda *v: (C.c_float * 3)(*v)
    inf, nan = float("inf"), float("nan")

    def integrate(panos=x, w2l=x, F=2, H=4, W=8, fov=26.9, lo=f3(0, 0, 0), step=f3(1, 1, 1), dims=(4, 5, 6), trunc=0.3, s=x, c=x):
        return L.lnh_tsdf_integrate(panos, w2l, F, H, W, 2.0, fov, 80.0, lo, step, *dims, trunc, s, c, None)

    cases = [(dict(panos=None), "null"), (dict(w2l=None), "null"), (dict(lo=None), "null"), (dict(step=None), "null"),
             (dict(s=None), "null"), (dict(c=None), "null"), (dict(F=0), "none may be 0"), (dict(H=0), "none may be 0"),
             (dict(W=0), "none may be 0"), (dict(dims=(1, 5, 6)), ">= 2"), (dict(dims=(4, 0, 6)), ">= 2"), (dict(dims=(4, 5, 1)), ">= 2"),
             (dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(trunc=inf), "trunc"), (dict(trunc=nan), "trunc"),
             (dict(step=f3(1, 0, 1)), "step[1]"), (dict(step=f3(-1, 1, 1)), "step[0]"), (dict(step=f3(1, 1, nan)), "step[2]"),
             (dict(step=f3(1, inf, 1)), "step[1]"), (dict(lo=f3(0, nan, 0)), "lo[1]"), (dict(fov=0.0), "fov")]
    for kw, word in cases:
        assert integrate(**kw) == INVALID_ARG and word in err(), (kw, err())
    for dims in ((1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 16, 2)):
        assert integrate(dims=dims) == UNSUPPORTED and "2^31" in err(), (dims, err())
    assert integrate(H=4097, W=4096) == UNSUPPORTED and "2^24" in err()
    assert integrate(H=1 << 16, W=1 << 16) == UNSUPPORTED and "2^24" in err()

    def finalize(s=x, c=x, dims=(4, 5, 6), mc=1, vol=x):
        return L.lnh_tsdf_finalize(s, c, *dims, mc, vol, None)

    for kw, word in ((dict(s=None), "null"), (dict(c=None), "null"), (dict(vol=None), "null"), (dict(dims=(4, 1, 6)), ">= 2"),
                     (dict(mc=0), "min_count")):
        assert finalize(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert finalize(dims=(1 << 11, 1 << 10, 1 << 10)) == UNSUPPORTED and "2^31" in err()

    def observed(v=x, V=10, c=x, dims=(4, 5, 6), mc=1, keep=x):
        return L.lnh_mesh_vertex_observed(v, V, c, *dims, mc, keep, None)

    for kw, word in ((dict(v=None), "null"), (dict(c=None), "null"), (dict(keep=None), "null"), (dict(V=0), "no vertices"),
                     (dict(dims=(4, 5, 0)), ">= 2"), (dict(mc=0), "min_count")):
        assert observed(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert observed(V=1 << 31) == UNSUPPORTED and "2^31" in err()
    assert observed(dims=(1 << 16, 1 << 16, 2)) == UNSUPPORTED and "2^31" in err()

    need = L.lnh_mesh_filter_workspace_size(300, 700)

    def count(keep=x, V=300, tri=x, T=700, ws=x, wsb=need, counts=x):
        return L.lnh_mesh_filter_count(keep, V, tri, T, ws, wsb, counts, None)

    def emit(v=x, keep=x, V=300, tri=x, T=700, ws=x, wsb=need, ov=x, mv=10, ot=x, mt=10):
        return L.lnh_mesh_filter_emit(v, keep, V, tri, T, ws, wsb, ov, mv, ot, mt, None)

    common = ((dict(keep=None), "null"), (dict(tri=None), "null"), (dict(ws=None), "null"), (dict(V=0), "empty mesh"),
              (dict(T=0), "empty mesh"), (dict(wsb=need - 4), "workspace"), (dict(wsb=0), "workspace"), (dict(ws=18), "workspace"),
              (dict(V=400), "workspace"), (dict(T=2000), "workspace"))
    for fn, own in ((count, ((dict(counts=None), "null"),)),
                    (emit, ((dict(v=None), "null"), (dict(ov=None), "null"), (dict(ot=None), "null"), (dict(mv=0), "capacity")))):
        for kw, word in common + own:
            assert fn(**kw) == INVALID_ARG and word in err(), (fn.__name__, kw, err())
        assert fn(V=1 << 31, wsb=1 << 62) == UNSUPPORTED and "2^31" in err()
        assert fn(T=1 << 31, wsb=1 << 62) == UNSUPPORTED and "2^31" in err()


# ------------------------------------------------------------------------------------------------- the restatement
def _small_case(seed=0, F_=5, H=6, W=16, dims=(5, 7, 9)):
    rng = np.random.default_rng(seed)
    panos = rng.uniform(1.0, 4.0, (F_, H, W)).astype(F)
    panos[rng.random(panos.shape) < 0.15] = 0
    poses = np.stack([ref.translation_pose(rng.uniform(-0.5, 0.5, 3)) for _ in range(F_)])
    w2l = np.stack([ref.inverse_affine(p) for p in poses])
    lo, step = F([-2.0, -2.5, -1.0]), F([1.0, 0.8, 0.25])
    return panos, w2l, (30.0, 60.0), lo, step, dims, F(1.5)


def test_frames_split_over_calls_give_the_bits_of_one_call():
    panos, w2l, K, lo, step, dims, trunc = _small_case()
    rng = np.random.default_rng(1)
    s0, c0 = rng.standard_normal(dims).astype(F), rng.integers(0, 5, dims).astype(np.uint32)  # earlier content
    s, c = ref.integrate(panos, w2l, *K, 80.0, lo, step, dims, trunc, s0, c0)
    assert (c > c0).sum() > 50 and (c == c0).sum() > 0 and (c - c0).max() == len(panos)
    for cut in (1, 2, 4):
        s1, c1 = ref.integrate(panos[:cut], w2l[:cut], *K, 80.0, lo, step, dims, trunc, s0, c0)
        s2, c2 = ref.integrate(panos[cut:], w2l[cut:], *K, 80.0, lo, step, dims, trunc, s1, c1)
        assert np.array_equal(s2.view(np.int32), s.view(np.int32)) and np.array_equal(c2, c)
    assert np.array_equal(s[c == c0].view(np.int32), s0[c == c0].view(np.int32))  # an unobserved point keeps its sum


def test_an_all_dropped_frame_changes_nothing():
    panos, w2l, K, lo, step, dims, trunc = _small_case()
    s, c = ref.integrate(panos, w2l, *K, 80.0, lo, step, dims, trunc, np.zeros(dims, F), np.zeros(dims, np.uint32))
    for value in (0.0, -1.0, np.nan, np.inf, -np.inf):
        dropped = np.full_like(panos[:1], value)
        s1, c1 = ref.integrate(dropped, w2l[:1], *K, 80.0, lo, step, dims, trunc, s, c)
        assert np.array_equal(s1.view(np.int32), s.view(np.int32)) and np.array_equal(c1, c), value
    mixed = np.insert(panos, 2, np.float32(-1.0), axis=0)
    s2, c2 = ref.integrate(mixed, np.insert(w2l, 2, w2l[0], axis=0), *K, 80.0, lo, step, dims, trunc, np.zeros(dims, F),
                           np.zeros(dims, np.uint32))
    assert np.array_equal(s2.view(np.int32), s.view(np.int32)) and np.array_equal(c2, c)


def test_the_wrap_closes_the_wedge_behind_the_sensor():
    """4 x 8 image: a column is pi/4 wide.  Points behind the sensor with a small negative y have beta just below 2 pi, which
    rounds to column 8 = W: lnh_lidar_to_pano drops such a return, the TSDF reads column 0 — as it does for their mirror images
    at small positive y."""
    H, W, K = 4, 8, (30.0, 60.0)
    panos = np.full((1, H, W), 5.0, F)
    lo, step, dims = F([-3.0, -0.3, -0.2]), F([1.0, 0.2, 0.2]), (2, 4, 3)  # y = -0.3, -0.1, 0.1, 0.3; x = -3, -2
    w2l = ref.inverse_affine(np.eye(4, dtype=F))[None]
    zeros = np.zeros(dims, F), np.zeros(dims, np.uint32)
    s_w, c_w = ref.integrate(panos, w2l, *K, 80.0, lo, step, dims, F(0.5), *zeros)
    s_n, c_n = ref.integrate(panos, w2l, *K, 80.0, lo, step, dims, F(0.5), *zeros, wrap=False)
    assert (c_n[:, :2] == 0).all() and (c_n[:, 2:] == 1).all()  # the wedge: y < 0 unobserved without the wrap
    assert (c_w == 1).all()
    assert np.array_equal(s_w[:, :2], s_w[:, :1:-1])  # mirror images see the same depth at the same distance
    px, py, pz = ref.lattice_axes(lo, step, dims)
    ok, pix, _ = ref.project(px + 0 * py + 0 * pz, py + 0 * px + 0 * pz, pz + 0 * px + 0 * py, H, W, *K, 80.0)
    assert ok.all() and (pix % W == 0).all()


def test_finalize_and_fill():
    s, c = F([[-0.5, 1.0], [3.0, 0.0]]), np.array([[1, 2], [3, 0]], np.uint32)
    assert np.array_equal(ref.finalize(s, c, 1), F([[0.5, -0.5], [-1.0, 1.0]]))
    assert np.array_equal(ref.finalize(s, c, 2), F([[1.0, -0.5], [-1.0, 1.0]]))
    assert np.array_equal(ref.finalize(s, c, 4), np.full((2, 2), ref.FILL))  # all unobserved: one value, nothing crosses


def test_vertex_mask_and_filter_restatement():
    count = np.zeros((3, 3, 3), np.uint32)
    count[0, 0, 0] = count[1, 0, 0] = count[1, 1, 0] = 2
    v = F([[0.5, 0, 0], [1, 0.5, 0], [1, 0, 0.5], [1, 0, 0], [2, 2, 2], [1.5, 0, 0], [-0.5, 0, 0], [np.nan, 0, 0], [0, 0, 2.5]])
    assert ref.vertex_observed(v, count, 1).tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 0]
    assert ref.vertex_observed(v, count, 3).tolist() == [0] * 9
    keep = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    tri = np.array([[0, 2, 3], [0, 1, 2], [5, 3, 2], [3, 4, 5], [0, 6, 2], [-1, 0, 2], [2, 2, 5]], np.int32)
    fv, ft = ref.mesh_filter(v[:6], keep, tri)
    assert np.array_equal(fv, v[[0, 2, 3, 5]]) and ft.tolist() == [[0, 1, 2], [3, 2, 1], [1, 1, 3]]


# ---------------------------------------------------------------------------------------------------------- the sphere
def test_sphere_vertices_lie_on_the_sphere():
    """One frame of constant depth d0 = 4 with an identity pose, h = 0.25, trunc = 3 h, K = (2.0, 26.9), 66 x 1030: inside the
    image's elevation band the volume is u = (r - d0) / trunc, a function of r alone.

    Interpolation.  Along a lattice edge r is convex with second derivative at most 1 / r, so linear interpolation between two ends
    h apart misplaces the zero of r - d0 by at most h^2 / 8 * max(1 / r) in r; both ends of a crossing edge have r >= d0 - h.
    That is h^2 / (8 (d0 - h)) = 2.083e-3.

    Rounding, from the header's operations (ulp(4..8) = 2^-21, so half of it is 2^-22):
      p, q        exact: every lattice coordinate is a multiple of 0.25 below 8, the matrix is the identity
      r           (q_x q_x + q_y q_y) + q_z q_z is exact (multiples of 1/16 below 128); the square root is rounded once: 2^-22
      s = d0 - r  exact (Sterbenz: r within [d0 / 2, 2 d0] wherever |s| <= trunc)
      s / trunc   one rounding of a quotient of magnitude <= 1: 2^-24 in u, trunc * 2^-24 in r;  -(sum / 1) is exact
      t           iso - va is exact; vb - va and the quotient round once each: 2 * 2^-24 relative on t <= 1, h * 2^-23 in r
                  (moving a point along an edge changes r by at most as much)
      float(i)+t  i < 64: half an ulp of [32, 64) is 2^-19 index units: h * 2^-19
      world       lo + v * step in float64, rounded to float32 once; the two other coordinates are lattice values: 2^-22
    A value error e in r at both ends of an edge moves the interpolant's zero by at most e in r.  Sum: 2^-22 + trunc 2^-24 +
    h 2^-23 + h 2^-19 + 2^-22 = 1.03e-6 (tsdf_ref.sphere_rounding_term)."""
    s = ref.sphere()
    v, t, parts = ref.extract_mesh(s["sum"], s["count"], s["lo"], s["step"])
    assert len(v) > 500 and len(t) > 500 and 0 < parts["keep"].sum() < len(parts["keep"])
    assert abs(ref.sphere_rounding_term() - 1.03e-6) < 1e-8
    err, bound, excess, allowed = ref.check_sphere_vertices(v)
    print(f"sphere: {len(v)} vertices, max |r - d0| {err:.3e} (bound {bound:.3e}); elevation excess {excess:.3f} pixels "
          f"(allowed {allowed:.3f})")
    assert abs(bound - 2.0844e-3) < 1e-6
    assert err <= bound
    assert allowed == 0.5 and excess <= allowed  # half a pixel wide of the image's elevation band at most
    # what the trim removed is the rim where observed free space meets the unobserved fill, not the sphere
    removed = parts["vertices"][parts["keep"] == 0]
    assert len(removed) > 0
    # normals face the sensor at the origin
    a, b, c = (v[t[:, k]].astype(np.float64) for k in range(3))
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3) < 0).all()


# -------------------------------------------------------------------------------------------------------- closed loop
def _cast(v, t):
    def cast(o, d):
        out = rc.cast_rays(v, t, o, d)
        return out["t_hit"], out["primitive_normals"]
    return cast


@pytest.mark.parametrize("drop", [0.0, 0.15])
def test_closed_loop_on_the_room(drop):
    """The issue's end-to-end condition on the method: fuse the four frames of the box room, mesh, cast 600 seeded rays back from
    two training poses.  Hit share >= 0.85, median |depth error| <= 0.1 h, 95th percentile <= 0.5 h, every hit normal faces the
    sensor.  The restatement's own figures (float32, this file): no drop 0.952 / 0.980, median 0.0076 h / 0.0108 h, 95th
    percentile 0.126 h / 0.161 h, maximum 0.45 h / 0.54 h; 15 % dropped 0.897 / 0.948, 95th percentile 0.171 h / 0.159 h."""
    r = ref.room(drop)
    assert r["dims"] == (66, 46, 29) and float(r["trunc"]) == float(F(3) * F(0.2))
    v, t, parts = ref.room_mesh(drop)
    assert len(t) > 5000
    for frame in (0, 1):
        share, err, facing = ref.closed_loop(_cast(v, t), frame, drop=drop)
        print(f"room drop {drop} frame {frame}: hit share {share:.3f}, median {np.median(err):.4f} h, 95th percentile "
              f"{np.percentile(err, 95):.4f} h, max {err.max():.3f} h, normals facing {facing}")
        assert share >= 0.85
        assert np.median(err) <= 0.1
        assert np.percentile(err, 95) <= 0.5
        assert facing


# ------------------------------------------------------------------------------------------------------ the Python side
def test_python_surface_and_no_cpu_fallback():
    from lidarnerf import nvs, tsdf
    sig = inspect.signature(tsdf.TSDFVolume.__init__)
    assert list(sig.parameters) == ["self", "box", "resolution", "voxel_size", "truncation", "device"]
    assert (sig.parameters["resolution"].default, sig.parameters["voxel_size"].default, sig.parameters["truncation"].default) == \
        (256, None, None)
    assert list(inspect.signature(tsdf.TSDFVolume.integrate).parameters) == ["self", "panos", "poses", "lidar_K", "max_depth"]
    for name in ("volume", "extract_mesh"):
        p = inspect.signature(getattr(tsdf.TSDFVolume, name)).parameters
        assert list(p) == ["self", "min_count"] and p["min_count"].default == 1
    assert list(inspect.signature(tsdf.TSDFVolume.scene).parameters)[:2] == ["self", "grid_resolution"]
    sig = inspect.signature(nvs.MeshNVS.fit)
    assert list(sig.parameters) == ["frames", "resolution", "voxel_size", "truncation", "box", "margin", "min_count", "max_depth",
                                    "intensity_interpolate_k", "grid_resolution"]
    assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "frames")
    assert sig.parameters["resolution"].default == 256 and sig.parameters["intensity_interpolate_k"].default == 5
    assert isinstance(inspect.getattr_static(nvs.MeshNVS, "fit"), classmethod)
    assert list(inspect.signature(nvs.MeshNVS.raydrop_dataset).parameters) == ["self", "frames"]
    assert "has no fit" not in nvs.__doc__ and "MeshNVS.fit" in nvs.__doc__
    with pytest.raises(ValueError, match="no frames"):
        nvs.MeshNVS.fit([])
    with pytest.raises(ValueError, match="max > min"):
        tsdf.TSDFVolume(([0, 0, 0], [1, 0, 1]))
    with pytest.raises(ValueError, match="resolution"):
        tsdf.TSDFVolume(([0, 0, 0], [1, 1, 1]), resolution=1)
    with pytest.raises(ValueError, match="voxel_size"):
        tsdf.TSDFVolume(([0, 0, 0], [1, 1, 1]), voxel_size=0.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tsdf.TSDFVolume(([0, 0, 0], [1, 1, 1]), resolution=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsdf.TSDFVolume(([0, 0, 0], [1, 1, 1]), resolution=8, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        tsdf.vertex_observed(torch.zeros(4, 3), torch.zeros(4, 4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        tsdf.filter_mesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.ones(4, dtype=torch.uint8))


def test_lattice_rule():
    lo, step, dims = ref.lattice_of([-1, -2, -3], [1, 2, 3], resolution=9)
    assert dims == (9, 9, 9) and np.array_equal(step, F([0.25, 0.5, 0.75])) and np.array_equal(lo, F([-1, -2, -3]))
    lo, step, dims = ref.lattice_of(ref.ROOM_LO - 0.55, ref.ROOM_HI + 0.55, voxel_size=0.2)
    assert dims == (66, 46, 29) and np.array_equal(step, F([0.2, 0.2, 0.2]))
    assert ref.lattice_of([0, 0, 0], [0.1, 1.0, 1.01], voxel_size=0.5)[2] == (2, 2, 3)
