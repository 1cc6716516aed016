"""Mesh export without a GPU: the generated case table (csrc/gen_mc_tables.py -> csrc/mc_tables.h) against its own rules, the
NumPy restatement of the output contract (tests/marching_cubes_ref.py) against what a mesh must be — closed, consistently
wound, dense matter inside —, the three entry points exported, declared and bound, every refusal before any launch, the PLY
writer, and the Python surface with its refusal of CPU tensors."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import marching_cubes_ref as ref
from marching_cubes_ref import gen_mc_tables as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2  # LNH_ERR_INVALID_ARG, LNH_ERR_UNSUPPORTED (include/lidarnerf_hip.h)
NAMES = ("lnh_marching_cubes_workspace_size", "lnh_marching_cubes_count", "lnh_marching_cubes_emit")


# ------------------------------------------------------------------------------------------------------- the table
def test_committed_table_is_what_the_generator_writes():
    path = os.path.join(ROOT, "lidar-nerf_amd", "csrc", "mc_tables.h")
    assert open(path, encoding="utf-8").read() == gen.header()
    assert gen.MAX_TRIANGLES == max(gen.TRI_COUNT) == 5 and gen.TRI_COUNT[0] == gen.TRI_COUNT[255] == 0
    text = open(os.path.join(ROOT, "lidar-nerf_amd", "csrc", "mesh.hip")).read()
    assert "static_assert(kMcMaxTriangles" in text and '#include "mc_tables.h"' in text


def test_triangles_use_exactly_the_crossing_edges():
    for case in range(256):
        want = [e for e, (a, b) in enumerate(gen.EDGES) if (case >> a & 1) != (case >> b & 1)]
        used = sorted({e for t in gen.TRIANGLES[case] for e in t})
        assert used == want, case
        assert all(len(set(t)) == 3 for t in gen.TRIANGLES[case]), case
    # numbering: edge 4 * axis + k runs along `axis` from its lower corner, the owner of its vertex
    for e, (lo, hi) in enumerate(gen.EDGES):
        axis, off = ref.edge_owner(e)
        assert hi == lo | 1 << axis and off[axis] == 0 and gen.CORNERS[lo] == off
    assert len(set(gen.EDGES)) == 12


def _face_rule(case, ring):
    """The face rule restated from the four bits alone, undirected: the set of {edge, edge} segments."""
    below = [case >> c & 1 for c in ring]
    side = lambda i, j: gen.edge_between(ring[i % 4], ring[j % 4])
    around = lambda i: frozenset((side(i, i - 1), side(i, i + 1)))  # cuts corner i off
    n = sum(below)
    if n in (0, 4):
        return set()
    if n == 1:
        return {around(below.index(1))}
    if n == 3:
        return {around(below.index(0))}
    if below[0] == below[2]:  # ambiguous: every below corner is cut off on its own
        return {around(i) for i in range(4) if below[i]}
    i = next(i for i in range(4) if below[i] and below[(i + 1) % 4])
    return {frozenset((side(i, i - 1), side(i + 1, i + 2)))}


def test_fans_leave_the_face_rules_segments_on_every_face():
    """What a cell shows its neighbour through a face is the set of triangle sides not cancelled inside the cell; it must be
    exactly the face rule's segments, which read only that face's four bits — so the neighbour shows the same."""
    edge_faces = {e: {f for f, (_, ring) in enumerate(gen.FACES) if set(gen.EDGES[e]) <= set(ring)} for e in range(12)}
    assert all(len(f) == 2 for f in edge_faces.values())
    ambiguous = 0
    for case in range(256):
        d = ref.directed_edge_counts(gen.TRIANGLES[case])
        left = {e for e in d if (e[1], e[0]) not in d}
        assert all(d[e] == 1 for e in d), case
        on_face = {f: set() for f in range(6)}
        for a, b in left:
            shared = edge_faces[a] & edge_faces[b]
            assert len(shared) == 1, (case, a, b)  # every side left over lies on one face
            on_face[shared.pop()].add(frozenset((a, b)))
        for f, (_, ring) in enumerate(gen.FACES):
            want = _face_rule(case, ring)
            ambiguous += len(want) == 2
            assert on_face[f] == want, (case, f)
            assert {frozenset(s) for s in gen.face_segments(case, gen.FACES[f])} == want
    assert ambiguous > 0


# ------------------------------------------------------------------------------------------------- the restatement
def test_all_256_cases_give_a_closed_consistently_wound_mesh():
    vol, iso = ref.case_volume()
    assert vol.shape == (64, 64, 4)
    cases = ref.cell_cases(ref.below_mask(vol, iso))
    assert sorted(cases[1::4, 1::4, 1].ravel().tolist()) == list(range(256))
    v, t, counts = ref.marching_cubes(vol, iso)
    assert counts == (len(v), len(t), 0, 0) and len(t) > 256 and v.dtype == np.float32 and t.dtype == np.int32
    assert ref.open_edges(t) == []  # every undirected edge: two triangles, once in each direction
    assert t.min() == 0 and t.max() == len(v) - 1 and len(np.unique(t)) == len(v)
    assert len(np.unique(v, axis=0)) == len(v)  # indexed: a shared vertex appears once
    # vertex order: lattice-point order of the owner, within a point x, y, z edge
    owner = np.floor(v).astype(np.int64)
    axis = np.argmax(v != np.floor(v), axis=1)
    key = np.ravel_multi_index(owner.T, vol.shape) * 3 + axis
    assert np.all(np.diff(key) > 0)
    assert ref.signed_volume(v, t) < 0  # the below blocks are holes in not-below matter: normals point into them


def test_random_volume_is_closed_off_the_boundary():
    rng = np.random.default_rng(5)
    vol = rng.standard_normal((12, 12, 12)).astype(np.float32)
    v, t, counts = ref.marching_cubes(vol, 0.1)
    assert counts[0] == len(v) > 500 and counts[1] == len(t)
    hi = np.array(vol.shape) - 1
    on_boundary = lambda a, b: bool(np.any((v[a] == 0) & (v[b] == 0)) or np.any((v[a] == hi) & (v[b] == hi)))
    assert ref.open_edges(t, skip=on_boundary) == []
    assert len(ref.open_edges(t)) > 0  # (the surface does reach the boundary)
    # every vertex lies on its edge, strictly past the lower end or on it
    frac = v - np.floor(v)
    assert np.all((frac != 0).sum(1) <= 1) and np.all(frac >= 0) and np.all(frac < 1)


def test_values_equal_to_iso_and_nan_are_not_below():
    vol = np.full((3, 3, 3), 1.0, np.float32)
    vol[1, 1, 1] = 0.0
    v, t, counts = ref.marching_cubes(vol, 0.0)  # the centre EQUALS iso: not below, nothing crosses
    assert counts == (0, 0, 0, 0) and v.shape == (0, 3) and t.shape == (0, 3)
    v, t, counts = ref.marching_cubes(vol, 1.0)  # the centre alone is below 1.0: six vertices, all at the far ends' t
    assert counts == (6, 8, 0, 0) and ref.open_edges(t) == []
    vol[1, 1, 1] = np.nan
    assert ref.marching_cubes(vol, 1.0)[2] == (0, 0, 1, 0)
    vol[0, 0, 0] = -np.inf
    assert ref.marching_cubes(vol, 1.0)[2][2] == 2


def test_sphere_of_dense_matter():
    vol, iso = ref.sphere_volume((24, 24, 24), 8.3)
    v, t, _ = ref.marching_cubes(vol, iso)
    assert ref.open_edges(t) == []
    assert ref.euler_characteristic(len(v), t) == 2
    volume = ref.signed_volume(v, t)
    print("sphere: signed volume", volume, "of", 4 / 3 * np.pi * 8.3 ** 3)
    assert volume > 0  # normals point out of the dense matter


# -------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_exported_declared_and_bound():
    from lidarnerf import _hip
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    L = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(L, name), name
        assert re.search(r"LNH_API (int|uint64_t) " + name + r"\(", text), name
    assert "Replaces extract_geometry / mcubes.marching_cubes, nerf/utils.py:169-184" in text
    assert "Replaces extract_geometry / mcubes.marching_cubes, nerf/utils.py:169-184" in \
        open(os.path.join(ROOT, "lidar-nerf_amd", "csrc", "mesh.hip")).read()
    P, U32, U64, F32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    assert _hip._SIGS["lnh_marching_cubes_count"] == [P, U32, U32, U32, F32, P, U64, P]
    assert _hip._SIGS["lnh_marching_cubes_emit"] == [P, U32, U32, U32, F32, P, U64, P, U32, P, U32]
    assert L.lnh_marching_cubes_count.argtypes == _hip._SIGS["lnh_marching_cubes_count"] + [P]  # the stream comes last
    assert L.lnh_marching_cubes_emit.argtypes == _hip._SIGS["lnh_marching_cubes_emit"] + [P]
    assert L.lnh_marching_cubes_workspace_size.restype is U64
    assert L.lnh_marching_cubes_workspace_size.argtypes == [U32, U32, U32]


REFUSED_SIZES = ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 16, 2),
                 (0xffffffff, 0xffffffff, 0xffffffff), (1 << 31, 2, 2))


def test_workspace_size_grows_with_the_volume():
    from lidarnerf import _hip
    size = _hip.lib().lnh_marching_cubes_workspace_size
    base = size(16, 16, 16)
    assert base >= 4 * 16 ** 3 and base % 16 == 0 and size(2, 2, 2) > 0
    assert size(17, 16, 16) >= base + 4 * 256 and size(16, 17, 16) == size(17, 16, 16) == size(16, 16, 17)
    assert size(256, 256, 256) >= 4 * 256 ** 3 and size(256, 256, 256) < 5 * 256 ** 3
    assert size(1 << 10, 1 << 10, (1 << 11) - 1) > 0  # just below 2^31 samples
    for dims in REFUSED_SIZES:
        assert size(*dims) == 0, dims


def test_every_refusal_comes_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    need = L.lnh_marching_cubes_workspace_size(8, 9, 10)
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced or a kernel is launched

    def count(vol=x, dims=(8, 9, 10), iso=0.5, ws=x, wsb=need, counts=x):
        return L.lnh_marching_cubes_count(vol, *dims, iso, ws, wsb, counts, None)

    def emit(vol=x, dims=(8, 9, 10), iso=0.5, ws=x, wsb=need, v=x, mv=100, t=x, mt=100):
        return L.lnh_marching_cubes_emit(vol, *dims, iso, ws, wsb, v, mv, t, mt, None)

    common = ((dict(vol=None), "null"), (dict(ws=None), "null"), (dict(dims=(1, 9, 10)), ">= 2"), (dict(dims=(8, 0, 10)), ">= 2"),
              (dict(dims=(8, 9, 1)), ">= 2"), (dict(iso=float("nan")), "NaN"), (dict(wsb=need - 4), "workspace"),
              (dict(wsb=0), "workspace"), (dict(ws=18), "workspace"), (dict(dims=(8, 9, 11)), "workspace"))
    for fn, own in ((count, ((dict(counts=None), "null"),)),
                    (emit, ((dict(v=None), "null"), (dict(t=None), "null"), (dict(mv=0), "capacity"), (dict(mt=0), "capacity")))):
        for kw, word in common + own:
            assert fn(**kw) == INVALID_ARG and word in err(), (fn.__name__, kw, err())
        for dims in ((1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 16, 2)):
            assert fn(dims=dims, wsb=1 << 62) == UNSUPPORTED and "2^31" in err(), (fn.__name__, dims, err())
    assert emit(mv=1 << 31) == UNSUPPORTED and "int32" in err()


# ------------------------------------------------------------------------------------------------------ the Python side
def test_write_ply_round_trips(tmp_path):
    from lidarnerf.nerf import mesh
    vol, iso = ref.sphere_volume((9, 10, 11), 3.2)
    v, t, _ = ref.marching_cubes(vol, iso)
    path = os.path.join(tmp_path, "sphere.ply")
    mesh.write_ply(path, v.astype(np.float64) * 0.37 - 1.0, t)  # (float64 in, as extract_geometry hands them over)
    got_v, got_t = ref.read_ply(path)
    assert np.array_equal(got_v, (v.astype(np.float64) * 0.37 - 1.0).astype(np.float32)) and np.array_equal(got_t, t)
    mesh.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    got_v, got_t = ref.read_ply(path)
    assert got_v.shape == (0, 3) and got_t.shape == (0, 3)


def test_python_surface_and_no_cpu_fallback():
    from lidarnerf.nerf import mesh
    from lidarnerf.nerf.train_step import LidarTrainer
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(mesh.extract_fields) == ["bound_min", "bound_max", "resolution", "query_func", "S"]
    assert inspect.signature(mesh.extract_fields).parameters["S"].default == 128
    assert names(mesh.extract_geometry) == ["bound_min", "bound_max", "resolution", "threshold", "query_func"]
    assert names(mesh.density_volume)[:4] == ["model", "resolution", "S", "fp16"]
    sig = inspect.signature(mesh.density_volume)
    assert sig.parameters["S"].default == 128 and sig.parameters["fp16"].default is True
    assert names(mesh.marching_cubes) == ["volume", "threshold"] and names(mesh.write_ply) == ["path", "vertices", "triangles"]
    sig = inspect.signature(LidarTrainer.save_mesh)
    assert list(sig.parameters) == ["self", "save_path", "resolution", "threshold", "ema"]
    assert (sig.parameters["resolution"].default, sig.parameters["threshold"].default, sig.parameters["ema"].default) == \
        (256, 10, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.marching_cubes(np.zeros((4, 4, 4), np.float32), 0.5)

    class _Field(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.register_buffer("aabb_infer", torch.tensor([-1.0, -1, -1, 1, 1, 1]))

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.density_volume(_Field(), 8)
