"""Nearest-neighbour search on the device (csrc/knn.hip, lidarnerf/knn.py) against the NumPy restatement of its contract
(tests/knn_ref.py, brute force over all points).

Indices, squared distances and means are compared BIT FOR BIT, always: subtractions, products and sums, each one IEEE fp32
operation on both sides (nothing is contracted: -ffp-contract=off), the mean one fp64 sum in rank order, one division and one
rounding.  No tolerance is used anywhere in this file."""
import faulthandler
import functools
import os
import re

import numpy as np
import pytest
import torch

import knn_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5ca1ab1e
KS = (1, 5, 9, 16)
QUERY_COUNTS = (1, 63, 64, 65, 257, 4099)
CLOUD_SIZES = (1, 2, 255, 256, 257, 4099)
PAST_ONE_TILE = (17, 19, 16)  # 5168 cells
ONE_TILE = (16, 16, 16)  # 4096 cells: exactly one tile of the scan
ONE_PAST_A_TILE = (1, 17, 241)  # 4097 cells: the second tile holds one cell
GRIDS = {"all_points": (1, 1, 1), "2x3x5": (2, 3, 5), "default": None, "past_one_scan_tile": PAST_ONE_TILE,
         "one_scan_tile": ONE_TILE, "one_past_a_scan_tile": ONE_PAST_A_TILE}


def _scan_tile():
    """kScanTile of csrc/scan.h: the cells one tile of the one-workgroup scan covers."""
    text = open(os.path.join(ROOT, "lidar-nerf_amd", "csrc", "scan.h")).read()
    m = re.search(r"kScanThreads = (\d+), kScanPerThread = (\d+), kScanTile = kScanThreads \* kScanPerThread;", text)
    return int(m.group(1)) * int(m.group(2))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _index(points, grid=None):
    from lidarnerf.knn import PointCloudIndex
    return PointCloudIndex(np.ascontiguousarray(points, np.float32), grid_resolution=grid)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _search(index, queries, k, valid=None):
    idx, d2 = index.search_knn(_gpu(queries), k, valid=None if valid is None else _gpu(valid))
    assert idx.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(queries), k)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _assert_same(got, want, what):
    for name, g, w in zip(("indices", "dist2"), got, want):
        diff = _bits(g) != _bits(w)
        assert not diff.any(), (what, name, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def _three_points():
    return np.array([[0.5, 1.5, -2.0], [0.5, 1.5, -2.0], [4.0, -1.0, 3.0]], np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(points, values, queries, indices, dist2, {k: mean}) of a cloud: the brute force at k = 16 computed once (the answer at a
    smaller k is its first k ranks), shared, read-only."""
    points = _three_points() if name == "three_points" else kr.clouds()[name]
    queries = kr.queries_for(points, QUERY_COUNTS[-1] if name == "uniform" else 600)
    rng = np.random.default_rng(len(points) + 3)
    values = rng.uniform(0, 255, len(points)).astype(np.float32)
    idx, d2 = kr.brute_force(points, queries, 16)
    means = {k: kr.mean_of(values, idx[:, :k]) for k in KS}
    for a in (points, values, queries, idx, d2) + tuple(means.values()):
        a.setflags(write=False)
    return points, values, queries, idx, d2, means


CLOUDS = ("uniform", "lattice", "duplicates", "flat", "far_cluster", "one_point", "three_points")


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("name", CLOUDS)
def test_the_whole_output_equals_the_brute_force_at_every_grid(name, grid):
    points, values, queries, idx, d2, means = _case(name)
    if grid == "past_one_scan_tile":
        assert np.prod(PAST_ONE_TILE) > _scan_tile() + 1000
    if grid == "one_scan_tile":
        assert np.prod(ONE_TILE) == _scan_tile()
    if grid == "one_past_a_scan_tile":
        assert np.prod(ONE_PAST_A_TILE) == _scan_tile() + 1
    index = _index(points, GRIDS[grid])
    assert GRIDS[grid] is None or index.grid == GRIDS[grid]
    assert index.N == len(points) and index.bounds == (tuple(points.min(0).tolist()), tuple(points.max(0).tolist()))
    print(f"{name} / {grid}: grid {index.grid} for {len(points)} points, {len(queries)} queries")
    dvalues, dq = _gpu(values), _gpu(queries)
    for k in KS:  # (k > N on the one-point and the three-point cloud)
        _assert_same(_search(index, queries, k), (idx[:, :k], d2[:, :k]), (name, grid, k))
        mean = index.mean_of_neighbours(dq, dvalues, k)
        assert mean.dtype == torch.float32 and mean.shape == (len(queries),)
        assert np.array_equal(_bits(mean.cpu().numpy()), _bits(means[k])), (name, grid, k, "mean")
    held = min(16, len(points))
    assert (idx[:, :held] >= 0).all() and (idx[:, held:] == -1).all()


@pytest.mark.parametrize("n", QUERY_COUNTS)
def test_query_counts_around_a_wave_and_a_workgroup(n):
    points, values, queries, idx, d2, means = _case("uniform")
    index = _index(points)
    _assert_same(_search(index, queries[:n], 5), (idx[:n, :5], d2[:n, :5]), n)
    empty = index.search_knn(torch.zeros((0, 3), device="cuda"), 5)
    assert empty[0].shape == (0, 5) and empty[1].shape == (0, 5) and empty[0].dtype == torch.int32
    assert index.mean_of_neighbours(torch.zeros((0, 3), device="cuda"), _gpu(values), 5).shape == (0,)


@functools.lru_cache(maxsize=None)
def _big():
    rng = np.random.default_rng(77)
    points = rng.uniform([-20, -20, -2], [20, 20, 4], (CLOUD_SIZES[-1], 3)).astype(np.float32)
    queries = kr.queries_for(points, 200)
    points.setflags(write=False), queries.setflags(write=False)
    return points, queries


@pytest.mark.parametrize("n", CLOUD_SIZES)
def test_cloud_sizes_around_a_wave_and_a_workgroup(n):
    points, queries = _big()
    want = kr.brute_force(points[:n], queries, 9)
    for grid in (None, (3, 2, 4)):
        _assert_same(_search(_index(points[:n], grid), queries, 9), want, (n, grid))


def test_valid_mask_non_finite_queries_and_guard_words_behind_every_output():
    from lidarnerf import _hip
    points, values, queries, idx, d2, means = _case("far_cluster")
    s = _index(points, (5, 4, 3))
    dvalues = _gpu(values)
    for n, k in ((1, 1), (65, 5), (600, 9), (600, 16), (257, 3)):
        q = queries[:n].copy()
        valid = np.ones(n, np.uint8)
        valid[::3] = 0
        if n > 8:
            q[1, 0], q[4, 1], q[7, 2], q[8] = np.nan, np.inf, -np.inf, np.nan
        live = valid.astype(bool) & np.isfinite(q).all(1)
        want_idx = np.where(live[:, None], idx[:n, :k], -1).astype(np.int32)
        want_d2 = np.where(live[:, None], d2[:n, :k], np.float32(np.inf)).astype(np.float32)
        want_mean = np.where(live, kr.mean_of(values, idx[:n, :k]), np.float32(0)).astype(np.float32)
        dq, dvalid = _gpu(q), _gpu(valid)
        guard = 16
        bufs = {name: torch.full((n * w + guard,), SENTINEL, dtype=torch.int32, device="cuda")
                for name, w in (("indices", k), ("dist2", k), ("mean", 1))}
        for skip in (None, "indices", "dist2"):
            ptr = lambda name: None if name == skip else bufs[name].data_ptr()
            _hip.call("lnh_knn_search", s.points.data_ptr(), s.N, s.box.data_ptr(), *s.grid, s.cell_start.data_ptr(),
                      s.sorted.data_ptr(), s.slabs.data_ptr(), dq.data_ptr(), dvalid.data_ptr(), n, k, dvalues.data_ptr(),
                      ptr("indices"), ptr("dist2"), ptr("mean"))
            torch.cuda.synchronize()
            for name, w, want in (("indices", k, want_idx), ("dist2", k, want_d2), ("mean", 1, want_mean)):
                raw = bufs[name].cpu().numpy()
                assert (raw[n * w:] == SENTINEL).all(), ("guard words overwritten", name, n, k)
                assert np.array_equal(raw[:n * w].view(np.uint32), _bits(want).reshape(-1)), (name, n, k, skip)
        # the same through the Python surface, with a bool mask
        got = s.search_knn(dq, k, valid=dvalid.bool())
        _assert_same((got[0].cpu().numpy(), got[1].cpu().numpy()), (want_idx, want_d2), (n, k, "bool mask"))
        assert np.array_equal(_bits(s.mean_of_neighbours(dq, dvalues, k, valid=dvalid).cpu().numpy()), _bits(want_mean))
    # the build through the C ABI: guard words behind cell_start, the slab arrays and the sorted rows survive
    L = _hip.lib()
    nx, ny, nz = s.grid
    cells, S = nx * ny * nz, nx + ny + nz
    ws = torch.empty(int(L.lnh_knn_workspace_size(s.N, nx, ny, nz)), dtype=torch.uint8, device="cuda")
    cs = torch.full((cells + 1 + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    slabs = torch.full((2 * S + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    rows = torch.full((4 * s.N + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    _hip.call("lnh_knn_build_count", s.points.data_ptr(), s.N, s.box.data_ptr(), nx, ny, nz, ws.data_ptr(), ws.numel(),
              cs.data_ptr(), slabs.data_ptr())
    _hip.call("lnh_knn_build_fill", s.points.data_ptr(), s.N, s.box.data_ptr(), nx, ny, nz, ws.data_ptr(), ws.numel(),
              cs.data_ptr(), rows.data_ptr())
    torch.cuda.synchronize()
    assert (cs[cells + 1:] == SENTINEL).all() and (slabs[2 * S:] == SENTINEL).all() and (rows[4 * s.N:] == SENTINEL).all()
    assert torch.equal(cs[:cells + 1], s.cell_start) and torch.equal(slabs[:2 * S], s.slabs.view(torch.int32))
    assert int(cs[0]) == 0 and int(cs[cells]) == s.N
    # what the build recorded is what the restatement's build records
    g = kr.Grid(points, s.grid)
    assert np.array_equal(_bits(s.slabs.cpu().numpy()), _bits(np.concatenate(g.smin + g.pmax)))
    flat = (g.cells[:, 0] * ny + g.cells[:, 1]) * nz + g.cells[:, 2]
    assert np.array_equal(np.diff(s.cell_start.cpu().numpy()), np.bincount(flat, minlength=cells))
    got_rows = rows[:4 * s.N].cpu().numpy().view(np.uint32).reshape(-1, 4)
    order = got_rows[:, 3]
    assert sorted(order.tolist()) == list(range(s.N)) and np.array_equal(got_rows[:, :3], _bits(points)[order])
    assert (np.diff(flat[order]) >= 0).all()  # sorted by cell


def test_two_builds_and_two_searches_give_identical_outputs():
    """The order of the points inside a cell is arrival order (it may differ between the builds); no output may depend on it."""
    for name in ("duplicates", "lattice"):
        points, values, queries, idx, d2, means = _case(name)
        a, b = _index(points, (6, 7, 3)), _index(points, (6, 7, 3))
        assert torch.equal(a.cell_start, b.cell_start) and torch.equal(a.slabs.view(torch.int32), b.slabs.view(torch.int32))
        for k in (1, 9):
            first, again, other = _search(a, queries, k), _search(a, queries, k), _search(b, queries, k)
            _assert_same(first, again, (name, k, "two searches"))
            _assert_same(first, other, (name, k, "two builds"))
            _assert_same(first, (idx[:, :k], d2[:, :k]), (name, k))
            ma, mb = (x.mean_of_neighbours(_gpu(queries), _gpu(values), k).cpu().numpy() for x in (a, b))
            assert np.array_equal(_bits(ma), _bits(mb)) and np.array_equal(_bits(ma), _bits(means[k]))


def test_search_captured_in_a_graph_equals_the_eager_call():
    faulthandler.dump_traceback_later(120, exit=True)  # this test's own time limit: a replay that hangs ends the run
    try:
        points, values, queries, idx, d2, means = _case("far_cluster")
        index = _index(points)
        dq, dvalues = _gpu(queries.copy()), _gpu(values)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            index.search_knn(dq, 5), index.mean_of_neighbours(dq, dvalues, 5)  # (warm-up on the side stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):  # one stream, two launches
                cap_idx, cap_d2 = index.search_knn(dq, 5)
                cap_mean = index.mean_of_neighbours(dq, dvalues, 5)
        torch.cuda.current_stream().wait_stream(stream)
        for t in (cap_idx, cap_d2, cap_mean):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same((cap_idx.cpu().numpy(), cap_d2.cpu().numpy()), (idx[:, :5], d2[:, :5]), "captured")
        assert np.array_equal(_bits(cap_mean.cpu().numpy()), _bits(means[5]))
        dq.copy_(_gpu(queries[::-1].copy()))  # other queries in the same buffer: the replay reads them
        graph.replay()
        torch.cuda.synchronize()
        _assert_same((cap_idx.cpu().numpy(), cap_d2.cpu().numpy()), (idx[::-1, :5], d2[::-1, :5]), "replayed on other queries")
        assert np.array_equal(_bits(cap_mean.cpu().numpy()), _bits(means[5][::-1]))
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_the_mean_is_the_rank_order_fp64_sum():
    points, values, queries, idx, d2, means = _case("uniform")
    index = _index(points)
    dq = _gpu(queries[:500])
    # values whose float32 sum depends on the order and on the width of the accumulator
    rng = np.random.default_rng(2)
    wild = (rng.uniform(1, 2, len(points)) * 10.0 ** rng.integers(-6, 7, len(points))).astype(np.float32)
    for k in KS:
        got = index.mean_of_neighbours(dq, _gpu(wild), k).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(kr.mean_of(wild, idx[:500, :k]))), k
    # a cloud whose values are all equal returns that value exactly
    for value in (0.1, 255.0, 1e-30, -3.3):
        same = np.full(len(points), value, np.float32)
        for k in (3, 5, 7, 16):
            got = index.mean_of_neighbours(dq, _gpu(same), k).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(same[:500])), (value, k)
    # values of any float dtype and shape [N, 1]
    got = index.mean_of_neighbours(dq, _gpu(wild.astype(np.float64)[:, None]), 5).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(kr.mean_of(wild, idx[:500, :5])))


def test_every_device_side_refusal_raises():
    from lidarnerf.knn import PointCloudIndex
    points = _three_points()
    for bad in (np.nan, np.inf, -np.inf):
        w = points.copy()
        w[2, 1] = bad
        with pytest.raises(ValueError, match="1 point coordinates are not finite"):
            PointCloudIndex(w)
    with pytest.raises(ValueError, match="empty cloud"):
        PointCloudIndex(torch.zeros((0, 3), device="cuda"))
    dp = _gpu(points)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            with pytest.raises(RuntimeError, match="capturing"):
                PointCloudIndex(dp)
    index = PointCloudIndex(dp)
    assert index.points.data_ptr() == dp.data_ptr() and index.device == dp.device  # a float32 GPU tensor is used as it is
    q = torch.zeros(4, 3, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search_knn(torch.zeros(4, 3), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search_knn(np.zeros((4, 3), np.float32), 1)
    for bad in (torch.zeros(4, 2, device="cuda"), torch.zeros(12, device="cuda"), torch.zeros(4, 3, dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match=r"\[Q, 3\]"):
            index.search_knn(bad, 1)
    for k in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            index.search_knn(q, k)
    for valid in (torch.ones(3, dtype=torch.bool, device="cuda"), torch.ones(4, device="cuda"), torch.ones((4, 1), dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError, match="valid must be"):
            index.search_knn(q, 1, valid=valid)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search_knn(q, 1, valid=torch.ones(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.mean_of_neighbours(q, torch.zeros(3), 1)
    for values in (torch.zeros(4, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError, match="values must be"):
            index.mean_of_neighbours(q, values, 1)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="the cloud on"):
            index.search_knn(torch.zeros(4, 3, device="cuda:1"), 1)
