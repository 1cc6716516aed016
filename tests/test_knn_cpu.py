"""Nearest-neighbour search without a GPU: the entry points exported, declared and bound, every refusal of the C entry points
before any launch, the Python surface with its refusals, and the ARGUMENT ITSELF — the NumPy restatement's grid walk with the
stopping rule of DESIGN §16 (tests/knn_ref.py) returns exactly what its brute force over all points returns, on clouds full of
ties, duplicates, empty slabs and flat axes, and the brute force agrees with a float64 k-d tree wherever the neighbours are not
nearly equidistant."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import knn_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2
NAMES = ("lnh_knn_workspace_size", "lnh_knn_bounds", "lnh_knn_build_count", "lnh_knn_build_fill", "lnh_knn_search")
GRIDS = ((1, 1, 1), (2, 3, 5), (8, 8, 8), (17, 19, 16))
KS = (1, 5, 9, 16)


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
    P, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
    assert _hip._SIGS["lnh_knn_bounds"] == [P, U32, P, U64, P]
    assert _hip._SIGS["lnh_knn_build_count"] == [P, U32, P, U32, U32, U32, P, U64, P, P]
    assert _hip._SIGS["lnh_knn_build_fill"] == [P, U32, P, U32, U32, U32, P, U64, P, P]
    assert _hip._SIGS["lnh_knn_search"] == [P, U32, P, U32, U32, U32, P, P, P, P, P, U32, U32, P, P, P, P]
    for name in NAMES[1:]:
        assert getattr(L, name).argtypes == _hip._SIGS[name] + [P]  # the stream comes last
    assert L.lnh_knn_workspace_size.restype is U64 and L.lnh_knn_workspace_size.argtypes == [U32, U32, U32, U32]
    # the header states the contract
    for phrase in ("d2 = ((dx * dx) + (dy * dy)) + (dz * dz)", "bit-identical to those of nx = ny = nz = 1", "smallest index"):
        assert phrase in text, phrase


def test_workspace_size():
    from lidarnerf import _hip
    size = _hip.lib().lnh_knn_workspace_size
    assert size(1, 1, 1, 1) > 0 and size(1, 1, 1, 1) % 16 == 0
    assert size(100, 16, 16, 16) >= 4 * 16 ** 3 + 8 * 48
    assert size(100, 17, 16, 16) > size(100, 16, 16, 16)
    assert size(100, 1024, 1024, 2) >= 4 * 1024 * 1024 * 2
    last = 0
    for n in (1, 100, 10 ** 4, 10 ** 6, 10 ** 8, (1 << 31) - 1):  # monotone in the number of points ...
        assert size(n, 4, 4, 4) >= last
        last = size(n, 4, 4, 4)
    last = 0
    for g in (1, 2, 5, 64, 333, 1024):  # ... and in the grid
        assert size(1000, g, g, 3) >= last  # (the partials of the bounds pass are the floor)
        last = size(1000, g, g, 3)
    assert size(1000, 64, 64, 3) > size(1000, 5, 5, 3) and size(1000, 1024, 1024, 3) > size(1000, 333, 333, 3)
    for args in ((0, 1, 1, 1), (1 << 31, 1, 1, 1), (3, 0, 1, 1), (3, 1, 1025, 1), (3, 1, 1, 0xffffffff)):
        assert size(*args) == 0, args


def test_every_refusal_comes_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced or a kernel is launched
    need = L.lnh_knn_workspace_size(100, 4, 5, 6)

    def bounds(p=x, N=100, ws=x, wsb=need, box=x):
        if wsb == need - 4:
            wsb = L.lnh_knn_workspace_size(N, 1, 1, 1) - 4  # (the bounds pass needs what a 1 x 1 x 1 grid needs)
        return L.lnh_knn_bounds(p, N, ws, wsb, box, None)

    def count(p=x, N=100, box=x, grid=(4, 5, 6), ws=x, wsb=need, cs=x, slabs=x):
        return L.lnh_knn_build_count(p, N, box, *grid, ws, wsb, cs, slabs, None)

    def fill(p=x, N=100, box=x, grid=(4, 5, 6), ws=x, wsb=need, cs=x, srt=x):
        return L.lnh_knn_build_fill(p, N, box, *grid, ws, wsb, cs, srt, None)

    def search(p=x, N=100, box=x, grid=(4, 5, 6), cs=x, srt=x, slabs=x, q=x, valid=None, Q=7, k=5, values=x, idx=x, d2=x, mean=x):
        return L.lnh_knn_search(p, N, box, *grid, cs, srt, slabs, q, valid, Q, k, values, idx, d2, mean, None)

    cloud = ((dict(p=None), INVALID_ARG, "null"), (dict(N=0), INVALID_ARG, "empty cloud"), (dict(N=1 << 31), UNSUPPORTED, "int32"))
    grid = ((dict(box=None), INVALID_ARG, "null"), (dict(grid=(0, 5, 6)), INVALID_ARG, ">= 1"), (dict(grid=(4, 5, 0)), INVALID_ARG, ">= 1"),
            (dict(grid=(4, 1025, 6)), UNSUPPORTED, "1024"), (dict(grid=(1025, 5, 6)), UNSUPPORTED, "1024"))
    work = ((dict(ws=None), INVALID_ARG, "workspace"), (dict(wsb=need - 4), INVALID_ARG, "workspace"), (dict(ws=18), INVALID_ARG, "workspace"))
    cases = ((bounds, cloud + work + ((dict(box=None), INVALID_ARG, "null"),)),
             (count, cloud + grid + work + ((dict(grid=(4, 5, 7)), INVALID_ARG, "workspace"), (dict(cs=None), INVALID_ARG, "null"),
                                            (dict(slabs=None), INVALID_ARG, "null"))),
             (fill, cloud + grid + work + ((dict(cs=None), INVALID_ARG, "null"), (dict(srt=None), INVALID_ARG, "null"),
                                           (dict(srt=24), INVALID_ARG, "16-byte"))),
             (search, cloud + grid + ((dict(cs=None), INVALID_ARG, "null"), (dict(srt=None), INVALID_ARG, "null"),
                                      (dict(slabs=None), INVALID_ARG, "null"), (dict(srt=24), INVALID_ARG, "16-byte"),
                                      (dict(k=0), INVALID_ARG, "1 ... 16"), (dict(k=17), INVALID_ARG, "1 ... 16"),
                                      (dict(values=None), INVALID_ARG, "go together"), (dict(mean=None), INVALID_ARG, "go together"),
                                      (dict(values=None, mean=None, idx=None, d2=None), INVALID_ARG, "no output"),
                                      (dict(q=None), INVALID_ARG, "null"), (dict(Q=1 << 31), UNSUPPORTED, "queries"))))
    for fn, rows in cases:
        for kw, code, word in rows:
            assert fn(**kw) == code and word in err(), (fn.__name__, kw, err())
    assert search(Q=0, q=None) == 0  # no queries: nothing to do, nothing launched
    assert search(Q=0, q=None, k=17) == INVALID_ARG  # ... but the arguments are still checked


# --------------------------------------------------------------------------------------------------------- the argument
@functools.lru_cache(maxsize=None)
def _case(name):
    """(points, queries, {k: brute force}) of a cloud: computed once, shared, read-only."""
    points = kr.clouds()[name]
    queries = kr.queries_for(points, 48)
    want = {k: kr.brute_force(points, queries, k) for k in KS}
    for a in (points, queries) + tuple(x for pair in want.values() for x in pair):
        a.setflags(write=False)
    return points, queries, want


@pytest.mark.parametrize("name", ["uniform", "lattice", "duplicates", "flat", "far_cluster", "one_point"])
def test_the_grid_walk_equals_the_brute_force_bit_for_bit(name):
    points, queries, want = _case(name)
    assert len(points) <= 3000
    early = 0
    for grid in GRIDS:
        g = kr.Grid(points, grid)
        for k in KS:
            stats = []
            idx, d2 = kr.grid_walk(g, queries, k, stats)
            assert np.array_equal(idx, want[k][0]), (name, grid, k)
            assert np.array_equal(d2.view(np.uint32), want[k][1].view(np.uint32)), (name, grid, k)
            early += sum(1 for _, seen in stats if seen < len(points))
    held = min(KS[-1], len(points))
    assert (want[16][0][:, :held] >= 0).all() and (want[16][0][:, held:] == -1).all() and np.isinf(want[16][1][:, held:]).all()
    if len(points) > 16:
        assert early > 0, "the stopping rule never stopped a walk early: the comparison would show nothing"


def test_ties_go_to_the_smaller_index_and_ranks_ascend():
    points = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, 1], [2, 0, 0]], np.float32)
    idx, d2 = kr.brute_force(points, np.zeros((1, 3), np.float32), 16)
    assert idx[0].tolist() == [0, 1, 2, 3, 4, 5, 6] + [-1] * 9 and d2[0, :7].tolist() == [1] * 6 + [4] and np.isinf(d2[0, 7:]).all()
    for grid in GRIDS:
        got = kr.grid_walk(kr.Grid(points, grid), np.zeros((1, 3), np.float32), 16)
        assert np.array_equal(got[0], idx) and np.array_equal(got[1].view(np.uint32), d2.view(np.uint32))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0]], np.float32)
    idx, d2 = kr.brute_force(points, bad, 2, valid=np.array([1, 1, 0], bool))
    assert (idx == -1).all() and np.isinf(d2).all()
    assert kr.mean_of(np.arange(7, dtype=np.float32), np.array([[0, 1, 2], [6, -1, -1], [-1, -1, -1]])).tolist() == [1, 6, 0]


@pytest.mark.parametrize("k", KS)
def test_the_brute_force_agrees_with_a_float64_kd_tree(k):
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(21)
    points = rng.uniform(-5, 5, (4000, 3)).astype(np.float32)
    queries = rng.uniform(-5.5, 5.5, (1000, 3)).astype(np.float32)
    d, want = spatial.cKDTree(points.astype(np.float64)).query(queries.astype(np.float64), k=k + 1)
    d2 = d * d
    clear = (np.diff(d2, axis=1) > 1e-5 * d2[:, 1:]).all(1)  # the first k + 1 squared distances pairwise well apart
    left_out = int((~clear).sum())
    print(f"k = {k}: {left_out} of 1000 queries left out (nearly equidistant neighbours)")
    assert left_out <= 10
    got, _ = kr.brute_force(points, queries, k)
    assert np.array_equal(got[clear], want[clear][:, :k])
    g = kr.Grid(points, (9, 10, 11))
    walked, _ = kr.grid_walk(g, queries[:200], k)
    assert np.array_equal(walked, got[:200])


# ------------------------------------------------------------------------------------------------------ the Python side
def test_python_surface_and_refusals_that_need_no_device():
    from lidarnerf import knn, nvs
    Index, NVS = knn.PointCloudIndex, nvs.MeshNVS
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(Index.__init__) == ["self", "points", "grid_resolution"]
    assert inspect.signature(Index.__init__).parameters["grid_resolution"].default is None
    assert names(Index.search_knn) == ["self", "queries", "k", "valid"]
    assert names(Index.mean_of_neighbours) == ["self", "queries", "values", "k", "valid"]
    assert names(knn.default_grid_resolution) == ["n_points", "box"]
    assert names(NVS.__init__) == ["self", "scene", "points", "point_intensities", "intensity_interpolate_k", "grid_resolution"]
    assert inspect.signature(NVS.__init__).parameters["intensity_interpolate_k"].default == 5
    assert names(NVS.predict_frame) == ["self", "lidar_K", "lidar_pose", "lidar_H", "lidar_W", "compact"]
    assert inspect.signature(NVS.predict_frame).parameters["compact"].default is True
    assert names(NVS.raydrop_features) == ["self", "lidar_K", "lidar_pose", "lidar_H", "lidar_W"]
    assert names(NVS.predict_frame_with_raydrop) == ["self", "lidar_K", "lidar_pose", "lidar_H", "lidar_W", "model"]
    p = np.zeros((4, 3), np.float32)
    for bad in (np.zeros((4, 2), np.float32), np.zeros(12, np.float32), np.zeros((4, 3), np.int32), np.zeros((0, 3), np.float32),
                torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="must be|empty cloud"):
            Index(bad)
    with pytest.raises(TypeError):
        Index([[0.0, 0, 0]])
    for grid in (0, -1, 1025, (1, 2), (1, 2, 0), (1, 2, 3.5), "8", True, (4, 4, 2000)):
        with pytest.raises(ValueError, match="grid_resolution"):
            Index(p, grid_resolution=grid)
    for queries in (torch.zeros(5, 3), np.zeros((5, 3), np.float32)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            knn.check_queries(queries)
    for k in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            knn._check_k(k)
    with pytest.raises(TypeError, match="RaycastingScene"):
        NVS(object(), p, np.zeros(4, np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Index(p)


def test_default_grid_resolution_rule():
    from lidarnerf.knn import DEFAULT_POINTS_PER_CELL as per_cell, MAX_CELLS_PER_AXIS, default_grid_resolution as rule
    cube = [0, 0, 0, 1, 1, 1]
    assert rule(1, cube) == (1, 1, 1)
    n = rule(int(1000 * per_cell), cube)
    assert n == (10, 10, 10)
    assert rule(10 ** 13, cube) == (MAX_CELLS_PER_AXIS,) * 3
    nx, ny, nz = rule(int(4000 * per_cell), [0, 0, 0, 4, 2, 1])
    assert nx > ny > nz >= 1 and abs(nx * ny * nz - 4000) < 1500  # cubic cells: the proportions of the box
    assert rule(100000, [0, 0, 0, 1, 1, 0])[2] == 1  # a flat cloud: one layer
    assert rule(50, [2, 2, 2, 2, 2, 2]) == rule(50, [0, 0, 0, 0, 0, 0])  # a single place: whatever it is, it is a valid grid
    for n_points, box in ((1, cube), (10 ** 9, [-1, -1, -1, 1, 1, 1]), (50, [2, 2, 2, 2, 2, 2]), (10 ** 7, [0, 0, 0, 1e-30, 1, 1e30])):
        assert all(1 <= n <= MAX_CELLS_PER_AXIS for n in rule(n_points, box))
