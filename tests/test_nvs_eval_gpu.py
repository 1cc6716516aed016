"""The NVS baselines' evaluation on the device (csrc/eval_nvs.hip, lidarnerf/nvs_eval.py) against tests/nvs_eval_ref.py.

Exact tier: depths from {0, 1, 2, 4, 5, 8, 10, 16, 25, 32, 62.5, 1000} and intensities k / 16.  Every count is an integer and
every float32 square and absolute difference a multiple of 2^-24 (the clamp 1e-3f is 2^-33 times an integer, but a difference
from a depth >= 1 is rounded to float32 first), with a total below 2^29: their fp64 sum is exact in any order, so counts, n,
the rectangle, both sums, rmse and mae are compared with ==.  The SSIM of identical images is exactly 1: the kernel forms
its products unfused (the library is built without contraction), so numerator and denominator are the same bits.

General tier: random depths in [0, 90], intensities in [0, 1].  The sums of n non-negative float32 terms, added in fp64 in
any order, lie within n 2^-52 relative of math.fsum's exactly rounded sum (at most n - 1 additions, each 2^-53 relative, and
fsum's own rounding); rmse and mae add 2 ulp (a division, a square root).  The SSIM is held to the running error bound of
nvs_eval_ref.ssim_error_bounds at unit roundoff 2^-53 against the exact rational evaluation: for the mean (ref.mean_bound: the
per-position bounds plus a sum of m terms in any order) and for every position of the small shape, each read through a mask of
its 7 pixels and so with the window's own data_range (the full frame's constants reach every position through the mean).

TILE names the SSIM kernel's workgroup tile (kNvsTile): the shapes put n - 6 on one tile, one tile +- 1 and two tiles + 1."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import nvs_eval_ref as ref
import tsdf_ref

pytestmark = pytest.mark.gpu
F = np.float32
TILE = 256
K = (2.0, 26.9)
GUARD = 8
EXACT_DEPTHS = np.array([0, 1, 2, 4, 5, 8, 10, 16, 25, 32, 62.5, 1000], F)
SHAPES = [(1, 7), (1, 8), (3, 5), (6, 16), (23, 37), (1, TILE + 6), (1, TILE + 5), (1, TILE + 7), (1, 2 * TILE + 7), (66, 1030)]


def _slot(name):
    from lidarnerf import _hip
    return _hip.NVS_SLOT_NAMES.index(name)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _exact_frame(H, W, seed):
    rng = np.random.default_rng(seed)
    gt, pd = rng.choice(EXACT_DEPTHS, (H, W)), rng.choice(EXACT_DEPTHS, (H, W))
    flat_g, flat_p = gt.reshape(-1), pd.reshape(-1)
    # pairs exactly on the three thresholds in both directions, and both clamps, wherever the frame has room
    pairs = [(5, 4), (4, 5), (25, 16), (16, 25), (62.5, 32), (32, 62.5), (0, 1000), (1000, 0), (0, 0), (1000, 1000)]
    for k, (a, b) in enumerate(pairs):
        at = k * flat_g.size // len(pairs)  # (distinct pixels from 10 pixels on; smaller frames keep the later pairs)
        flat_g[at], flat_p[at] = a, b
    gi, pi = (rng.integers(0, 17, (H, W)) / 16).astype(F), (rng.integers(0, 17, (H, W)) / 16).astype(F)
    return gt.astype(F), pd.astype(F), gi, pi


def _random_frame(H, W, seed):
    rng = np.random.default_rng(seed)
    gt, pd = rng.uniform(0, 90, (H, W)).astype(F), rng.uniform(0, 90, (H, W)).astype(F)
    gt[rng.random((H, W)) < 0.1] = 0
    pd[rng.random((H, W)) < 0.1] = 0
    return gt, pd, rng.random((H, W), F), rng.random((H, W), F)


def _guarded(values, dtype):
    """A device buffer with GUARD sentinel words on either side of `values`: (whole buffer, the view in the middle)."""
    values = torch.as_tensor(values, dtype=dtype).reshape(-1)
    whole = torch.full((values.numel() + 2 * GUARD,), 77, dtype=dtype, device="cuda")
    whole[GUARD:GUARD + values.numel()] = values.cuda()
    return whole, whole[GUARD:GUARD + values.numel()]


def _guards_intact(whole):
    return bool((whole[:GUARD] == 77).all()) and bool((whole[-GUARD:] == 77).all())


POINTS_ROW = (0.375, 0.625, 0.5, 0.75, 0.125, 0.25, 11.0, 13.0, 1.0, 0.0)  # an LNH_PTS_* row: chamfer, fscore, ..., bad


def _device_rows(H, W, frames, max_frames=4, points_row=POINTS_ROW):
    """The three entry points on raw guarded buffers with a NaN-filled workspace: every (gt, pd, gi, pi, mask, scale) of
    `frames` into one accumulator.  Returns its state [1 + max_frames + 1, SLOTS] (the last row lies behind the history)."""
    from lidarnerf import _hip
    L = _hip.lib()
    need = int(L.lnh_nvs_eval_workspace_bytes(H, W))
    assert need > 0 and need % 8 == 0
    ws_whole, ws = _guarded(torch.full((need // 8,), math.nan, dtype=torch.float64), torch.float64)
    st_whole, st = _guarded(torch.zeros((1 + max_frames + 1) * _hip.NVS_SLOTS, dtype=torch.float64), torch.float64)
    st[(1 + max_frames) * _hip.NVS_SLOTS:] = -5.0  # the row behind the history
    row_whole, row = _guarded(torch.tensor(points_row, dtype=torch.float64), torch.float64)
    held = [ws_whole, st_whole, row_whole]
    for gt, pd, gi, pi, mask, scale in frames:
        bufs = [_guarded(torch.from_numpy(np.ascontiguousarray(a)), torch.float32) for a in (gt, pd, gi, pi)]
        m_whole, m = (None, None) if mask is None else _guarded(torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)), torch.uint8)
        mp = None if m is None else m.data_ptr()
        _hip.call("lnh_nvs_eval_frame", bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), bufs[3][1].data_ptr(),
                  mp, H, W, float(scale), ws.data_ptr(), need)
        _hip.call("lnh_nvs_eval_ssim", bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), mp, H, W, ws.data_ptr(), need)
        _hip.call("lnh_nvs_eval_finalize", H, W, ws.data_ptr(), need, row.data_ptr(), st.data_ptr(),
                  st[_hip.NVS_SLOTS:].data_ptr(), max_frames)
        torch.cuda.synchronize()
        for (whole, view), a in zip(bufs, (gt, pd, gi, pi)):
            assert _guards_intact(whole) and np.array_equal(view.cpu().numpy(), np.asarray(a, F).reshape(-1))  # inputs unchanged
        assert m_whole is None or _guards_intact(m_whole)
    assert all(_guards_intact(w) for w in held)
    return st.cpu().numpy().reshape(1 + max_frames + 1, _hip.NVS_SLOTS)


def _check_exact(row, want, rect, scale_note=""):
    """One row against the contract restatement where everything is exact."""
    n = want["n"]
    assert row[_slot("n")] == n and tuple(row[_slot("crop_r0"):_slot("crop_w") + 1]) == rect, (row, rect)
    assert row[_slot("sum_sq")] == want["sum_sq"] and row[_slot("sum_abs")] == want["sum_abs"], scale_note
    assert row[_slot("depth_rmse")] == math.sqrt(want["sum_sq"] / n) and row[_slot("intensity_mae")] == want["sum_abs"] / n
    for k, key in enumerate(("depth_a1", "depth_a2", "depth_a3")):
        assert row[_slot(key)] == want["counts"][k] / n, key
    assert row[_slot("data_range")] == want["data_range"]
    assert row[_slot("chamfer")] == POINTS_ROW[0] and row[_slot("f_score")] == POINTS_ROW[1] and row[_slot("frames")] == 1


def _ssim_close(row, want):
    """The kernel forms the per-position S of the contract restatement operation for operation (IEEE fp64 on both sides); the
    means differ by the order of a sum of m terms."""
    S = want["S"]
    if S.size == 0:
        assert math.isnan(row[_slot("depth_ssim")])
        return
    bound = ref.mean_bound(float(np.abs(S).sum()), np.zeros(S.size))
    assert abs(row[_slot("depth_ssim")] - want["depth_ssim"]) <= bound, (row[_slot("depth_ssim")], want["depth_ssim"], bound)


@pytest.mark.parametrize("H,W", SHAPES)
def test_exact_tier_every_shape(H, W):
    gt, pd, gi, pi = _exact_frame(H, W, 100 + W)
    want = ref.evaluate(gt, pd, gi, pi)
    ones = np.ones((H, W), np.uint8)
    state = _device_rows(H, W, [(gt, pd, gi, pi, None, 1.0)])
    again = _device_rows(H, W, [(gt, pd, gi, pi, None, 1.0)])
    with_mask = _device_rows(H, W, [(gt, pd, gi, pi, ones, 1.0)])
    assert state.tobytes() == again.tobytes() == with_mask.tobytes()  # twice, and NULL == all-ones, bit for bit
    row = state[1]
    _check_exact(row, want, (0, 0, H, W))
    _ssim_close(row, want)
    assert row[_slot("bad")] == 0 and np.array_equal(state[0], row)  # (0 + row)
    assert np.all(state[2:5] == 0) and np.all(state[5] == -5.0)
    if H * W >= 10:
        assert 0 < want["counts"][0] < want["counts"][1] < want["counts"][2] < H * W  # the threshold pairs tell the three apart
    # identical images
    same = _device_rows(H, W, [(gt, gt, gi, gi, None, 1.0)])[1]
    assert same[_slot("depth_rmse")] == 0 and same[_slot("intensity_mae")] == 0 and same[_slot("depth_ssim")] == 1.0
    assert same[_slot("depth_a1")] == same[_slot("depth_a2")] == same[_slot("depth_a3")] == 1.0 and same[_slot("bad")] == 0


def test_threshold_pairs_stay_out_of_the_strict_comparison():
    gt = np.array([[5, 4, 25, 16, 62.5, 32, 4]], F)
    pd = np.array([[4, 5, 16, 25, 32, 62.5, 4]], F)
    row = _device_rows(1, 7, [(gt, pd, gt * 0, gt * 0, None, 1.0)])[1]
    # thresh = 1.25 twice, 1.5625 twice, 1.953125 twice, 1 once
    assert [row[_slot(k)] for k in ("depth_a1", "depth_a2", "depth_a3")] == [1 / 7, 3 / 7, 5 / 7]
    clamps = np.array([[0, 1000, 0, 1000, 1e-3, 80, 79.99]], F)
    other = np.array([[1000, 0, 0, 1000, 0, 1000, 1e-4]], F)
    row = _device_rows(1, 7, [(clamps, other, gt * 0, gt * 0, None, 1.0)])[1]
    want = ref.evaluate(clamps, other, gt * 0, gt * 0)
    _check_exact(row, want, (0, 0, 1, 7))
    assert want["counts"] == [4, 4, 4] and want["data_range"] == float(F(80) - F(1e-3))


def _mask(H, W, r0, c0, h, w):
    m = np.zeros((H, W), np.uint8)
    m[r0:r0 + h, c0:c0 + w] = 1
    return m


def test_masks_crop_like_the_reference_and_bad_frames_are_marked():
    H, W = 23, 37
    gt, pd, gi, pi = _exact_frame(H, W, 9)
    for rect in ((0, 0, 5, 9), (0, 28, 5, 9), (18, 0, 5, 9), (18, 28, 5, 9), (4, 3, 1, 7), (22, 30, 1, 7), (2, 1, 20, 35)):
        mask = _mask(H, W, *rect)
        mask[mask != 0] = 1 + (np.arange(int(mask.sum())) % 200)  # any non-zero byte counts
        want = ref.evaluate(gt, pd, gi, pi, mask)  # (run.py's crop: intensities times 255)
        row = _device_rows(H, W, [(gt, pd, gi, pi, mask, 255.0)])[1]
        _check_exact(row, want, rect)
        _ssim_close(row, want)
        assert row[_slot("bad")] == 0 and want["n"] == rect[2] * rect[3]
    ell = np.zeros((H, W), np.uint8)
    ell[2:6, 3] = ell[5, 3:9] = 1
    for mask, n, rect in ((_mask(H, W, 7, 7, 2, 3), 6, (7, 7, 2, 3)), (ell, 9, (2, 3, 4, 6)), (np.zeros((H, W), np.uint8), 0, (0, 0, 0, 0))):
        state = _device_rows(H, W, [(gt, pd, gi, pi, mask, 255.0)])
        row = state[1]
        assert row[_slot("bad")] == 1 and state[0][_slot("bad")] == 1 and row[_slot("n")] == n
        assert tuple(row[_slot("crop_r0"):_slot("crop_w") + 1]) == rect
    assert math.isnan(_device_rows(H, W, [(gt, pd, gi, pi, _mask(H, W, 7, 7, 2, 3), 255.0)])[1][_slot("depth_ssim")])
    # a constant ground truth: data_range 0, C1 = C2 = 0, no variance on its side
    const = np.full((H, W), 8, F)
    flat = _device_rows(H, W, [(const, np.full((H, W), 4, F), gi, pi, None, 1.0)])[1]
    assert not math.isfinite(flat[_slot("depth_ssim")]) and flat[_slot("bad")] == 1 and flat[_slot("data_range")] == 0
    wavy = (1 + np.arange(H * W) % 3).astype(F).reshape(H, W)  # no window of 7 is constant
    row = _device_rows(H, W, [(const, wavy, gi, pi, None, 1.0)])[1]
    assert math.isfinite(row[_slot("depth_ssim")]) and row[_slot("bad")] == 0
    _ssim_close(row, ref.evaluate(const, wavy, gi, pi))
    # a bad points row marks the frame bad
    bad_points = POINTS_ROW[:9] + (1.0,)
    assert _device_rows(H, W, [(gt, pd, gi, pi, None, 1.0)], points_row=bad_points)[1][_slot("bad")] == 1
    nan_points = (math.nan,) + POINTS_ROW[1:]
    assert _device_rows(H, W, [(gt, pd, gi, pi, None, 1.0)], points_row=nan_points)[1][_slot("bad")] == 1


def test_accumulation_and_history():
    H, W = 23, 37
    frames = [_exact_frame(H, W, s) + (None, 1.0) for s in (1, 2, 3)]
    singles = [_device_rows(H, W, [f])[1] for f in frames]
    state = _device_rows(H, W, frames, max_frames=2)
    assert np.array_equal(state[1], singles[0]) and np.array_equal(state[2], singles[1])
    assert np.all(state[3] == -5.0)  # the third frame is past max_frames: the memory behind the history is untouched
    assert np.array_equal(state[0], (singles[0] + singles[1]) + singles[2]) and state[0][_slot("frames")] == 3
    none = _device_rows(H, W, frames[:1], max_frames=0)
    assert np.array_equal(none[0], singles[0]) and np.all(none[1] == -5.0)


@pytest.mark.parametrize("H,W", [(23, 37), (66, 1030)])
def test_general_tier(H, W):
    gt, pd, gi, pi = _random_frame(H, W, 31)
    want = ref.evaluate(gt, pd, gi, pi)
    n = H * W
    state = _device_rows(H, W, [(gt, pd, gi, pi, None, 1.0)])
    assert state.tobytes() == _device_rows(H, W, [(gt, pd, gi, pi, None, 1.0)]).tobytes()
    row = state[1]
    assert row[_slot("n")] == n and row[_slot("bad")] == 0 and row[_slot("data_range")] == want["data_range"]
    for k, key in enumerate(("depth_a1", "depth_a2", "depth_a3")):
        assert row[_slot(key)] == want["counts"][k] / n
    rel = n * 2.0 ** -52
    shares = {}
    for got, exact, extra in ((row[_slot("sum_sq")], want["sum_sq"], 0), (row[_slot("sum_abs")], want["sum_abs"], 0),
                              (row[_slot("depth_rmse")], want["depth_rmse"], 2), (row[_slot("intensity_mae")], want["intensity_mae"], 2)):
        bound = (rel + extra * 2.0 ** -52) * exact
        assert abs(got - exact) <= bound
        shares[len(shares)] = abs(got - exact) / bound
    print(f"{H} x {W}: sums use {max(shares.values()):.3g} of n 2^-52")
    _ssim_close(row, want)
    if n > 2000:  # (the rational model is slow: the small shape carries it)
        return
    g, p = ref.clamp(gt), ref.clamp(pd)
    exact = ref.ssim_exact(g, p, want["data_range"])
    bounds = ref.ssim_error_bounds(g, p, want["data_range"], ref.U64)
    assert None not in exact and np.all(np.isfinite(bounds))
    mean = sum(exact) / len(exact)
    mean_bound = ref.mean_bound(float(sum(abs(e) for e in exact)), bounds)
    err = abs(float(Fraction(float(row[_slot("depth_ssim")])) - mean))
    assert err <= mean_bound
    # per-position S, EVERY position of the sequence: a mask of its 7 pixels makes a sequence of one position.  Its data_range
    # is then the window's own (the bound is formed with it); the full frame's C1 and C2 enter every position through the mean
    # above.  Windows that straddle two image rows are no rectangle of 23 x 37, so the sweep presents the same row-major
    # sequence as 1 x 851; the rectangle addressing of windows inside a row is read on 23 x 37 itself at eight places.
    got = _sweep_positions(gt.reshape(-1), pd.reshape(-1))
    assert got.shape == (n - 6,)
    share = 0.0
    for q in range(n - 6):
        x, y = g[q:q + 7], p[q:q + 7]
        R = ref.data_range(x)
        b = ref.ssim_error_bounds(x, y, R, ref.U64)[0]
        e = abs(float(Fraction(float(got[q])) - ref.ssim_exact(x, y, R)[0]))
        assert e <= b, (q, e, b)
        share = max(share, e / b)
    for r, c in ((0, 0), (0, 30), (5, 11), (11, 3), (22, 0), (22, 30), (13, 17), (7, 29)):
        one = _device_rows(H, W, [(gt, pd, gi, pi, _mask(H, W, r, c, 1, 7), 1.0)])[1][_slot("depth_ssim")]
        assert one == got[r * W + c]  # the same window through the other addressing: the same bits
    print(f"{H} x {W}: SSIM mean uses {err / mean_bound:.3g} of its bound ({mean_bound:.3g}), a position at most {share:.3g} "
          f"(all {n - 6} positions)")


def _sweep_positions(gt_flat, pd_flat):
    """S of every position of a sequence [n], each read as the one-position SSIM of a 1 x n frame masked to its 7 pixels: all
    frames go into one accumulator with n - 6 rows of history, read once."""
    from lidarnerf import _hip
    n = gt_flat.size
    m = n - 6
    need = int(_hip.lib().lnh_nvs_eval_workspace_bytes(1, n))
    ws = torch.full((need // 8,), math.nan, dtype=torch.float64, device="cuda")
    state = torch.zeros((1 + m, _hip.NVS_SLOTS), dtype=torch.float64, device="cuda")
    row = torch.tensor(POINTS_ROW, dtype=torch.float64, device="cuda")
    g, p = torch.from_numpy(np.ascontiguousarray(gt_flat)).cuda(), torch.from_numpy(np.ascontiguousarray(pd_flat)).cuda()
    zero = torch.zeros_like(g)
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for q in range(m):
        mask.zero_()
        mask[q:q + 7] = 1
        _hip.call("lnh_nvs_eval_frame", g.data_ptr(), p.data_ptr(), zero.data_ptr(), zero.data_ptr(), mask.data_ptr(), 1, n, 1.0,
                  ws.data_ptr(), need)
        _hip.call("lnh_nvs_eval_ssim", g.data_ptr(), p.data_ptr(), mask.data_ptr(), 1, n, ws.data_ptr(), need)
        _hip.call("lnh_nvs_eval_finalize", 1, n, ws.data_ptr(), need, row.data_ptr(), state.data_ptr(), state[1:].data_ptr(), m)
    host = state.cpu().numpy()
    assert host[0, _slot("frames")] == m and host[0, _slot("bad")] == 0
    assert np.array_equal(host[1:, _slot("crop_c0")], np.arange(m)) and np.all(host[1:, _slot("n")] == 7)
    return host[1:, _slot("depth_ssim")]


# --------------------------------------------------------------------------------------------------- the Python layer
def _room_frames(H, W, sensors=tsdf_ref.ROOM_SENSORS, drop=0.0):
    """Ground-truth frame dicts of the box room (tests/tsdf_ref.py) with the keys of extract_dataset_frame that matter."""
    frames = []
    for k, s in enumerate(sensors):
        pano = tsdf_ref.room_depths(s, H, W, *tsdf_ref.ROOM_K)
        if drop:
            pano = np.where(np.random.default_rng(k).random((H, W)) < drop, F(0), pano).astype(F)
        z = pano * tsdf_ref.pixel_directions(H, W, *tsdf_ref.ROOM_K)[..., 2].astype(F) + F(s[2])
        frames.append({"pano": pano, "intensities": np.where(pano != 0, 0.5 + 0.1 * z, 0).astype(F),
                       "lidar_pose": tsdf_ref.translation_pose(s), "lidar_K": tsdf_ref.ROOM_K, "lidar_H": H, "lidar_W": W})
    return frames


@functools.lru_cache(maxsize=None)
def _mesh_nvs():
    from lidarnerf.nvs import MeshNVS
    return MeshNVS.fit(_room_frames(16, 64), voxel_size=0.4)


def _checker(H, W):
    return ((torch.arange(H, device="cuda")[:, None] + torch.arange(W, device="cuda")[None, :]) % 3 != 0)


def _pcgen_nvs(raycasting, H, W):
    from lidarnerf.nvs import PointCloudNVS
    mesh = _mesh_nvs()
    keep = _checker(H, W).reshape(-1, 1).float()
    return PointCloudNVS(mesh.points, mesh.point_intensities, raycasting=raycasting, raydrop=lambda rows: keep)


def _mesh_model(H, W):
    board = _checker(H, W)
    return lambda images: torch.where(board, 1.0, -1.0).reshape(1, 1, H, W)


def _gt_cloud(frame):
    from lidarnerf import convert
    return convert.pano_to_lidar(torch.from_numpy(frame["pano"]).cuda(), frame["lidar_K"])


def test_point_slots_equal_the_points_evaluator_and_the_clouds_the_predicted_ones():
    from lidarnerf import _hip, metrics
    from lidarnerf.nvs import NVSFrameEvaluator
    H, W = 6, 16
    gts = _room_frames(H, W, drop=0.1)
    for nvs, kw in ((_pcgen_nvs("cp", H, W), {}), (_pcgen_nvs("fpa", H, W), {}), (_mesh_nvs(), dict(model=_mesh_model(H, W)))):
        ev = NVSFrameEvaluator(H, W, K)
        pts = metrics.FramePointsEvaluator(H, W, 1.0, K)
        for gt in gts[:2]:
            pd = nvs.predict_frame_with_raydrop(gt["lidar_K"], gt["lidar_pose"], H, W, **kw)
            assert pd["local_points"].shape[0] > 10
            ev.update(gt, {"pano": pd["pano"], "intensities": pd["intensities"]})  # no cloud: the pano is back-projected
            count = int(ev.points.counts[0])
            assert count == pd["local_points"].shape[0]
            assert torch.equal(_bits(ev.points.clouds[0, :count, :3]), _bits(pd["local_points"]))
            assert torch.equal(_bits(ev.points.clouds[1, :int(ev.points.counts[1]), :3]), _bits(_gt_cloud(gt)))
            gt3 = torch.stack([torch.ones(H, W), torch.zeros(H, W), torch.from_numpy(gt["pano"])], -1).cuda()
            pts.update(pd["pano"], gt3)
        acc, rows = ev.rows()
        _, prow = pts.rows()
        assert rows.shape == (2, _hip.NVS_SLOTS) and prow.shape == (2, _hip.PTS_SLOTS)
        assert np.array_equal(rows[:, _slot("chamfer")], prow[:, 0]) and np.array_equal(rows[:, _slot("f_score")], prow[:, 1])
        assert np.all(np.isfinite(rows)) and acc[_slot("bad")] == 0


@pytest.mark.parametrize("kind", ["cp", "mesh"])
def test_the_loop_body_with_ray_drop_reads_nothing_back(kind):
    """What evaluate_nvs does per frame with raydrop=True — predict_images_with_raydrop and update — under the synchronisation
    check, for a point-cloud baseline and the mesh; the images are predict_frame_with_raydrop's."""
    from lidarnerf.nvs import NVSFrameEvaluator
    H, W = 6, 16
    gt = _room_frames(H, W, drop=0.1)[1]
    nvs, kw = (_pcgen_nvs("cp", H, W), {}) if kind == "cp" else (_mesh_nvs(), dict(model=_mesh_model(H, W)))
    pose = torch.from_numpy(gt["lidar_pose"]).cuda()
    gt_dev = {k: torch.from_numpy(gt[k]).cuda() for k in ("pano", "intensities")}
    full = nvs.predict_frame_with_raydrop(K, pose, H, W, **kw)
    ev = NVSFrameEvaluator(H, W, K)
    ev.update(gt_dev, nvs.predict_images_with_raydrop(K, pose, H, W, **kw))  # (allocations warmed)
    ev.clear()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lean = nvs.predict_images_with_raydrop(K, pose, H, W, **kw)
        ev.update(gt_dev, lean)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert "local_points" not in lean
    assert torch.equal(_bits(lean["pano"]), _bits(full["pano"])) and torch.equal(_bits(lean["intensities"]), _bits(full["intensities"]))
    count = int(ev.points.counts[0])
    assert count == full["local_points"].shape[0] and torch.equal(_bits(ev.points.clouds[0, :count, :3]), _bits(full["local_points"]))
    assert math.isfinite(ev.measure()["chamfer"])


@pytest.mark.parametrize("kind", ["cp", "fpa", "mesh", "mesh_plain"])
def test_evaluate_nvs_equals_frame_by_frame_eval_points_and_pano(kind, capsys):
    """The loop against the drop-in on the compact=True outputs, frame by frame.  The fitted MeshNVS carries a stored ray-drop
    U-Net, which needs 16 rows: its frames are 16 x 32, the point-cloud baselines' 6 x 16."""
    from lidarnerf import nvs as nvs_mod, nvs_eval
    H, W = (16, 32) if kind.startswith("mesh") else (6, 16)
    gts = _room_frames(H, W, drop=0.1)
    raydrop = kind != "mesh_plain"
    if kind.startswith("mesh"):
        import unet_ref
        from lidarnerf.unet import RayDropUNet
        nvs = _mesh_nvs()
        net = RayDropUNet()
        net.load_state_dict(unet_ref.hash_state_dict())
        net = net.cuda().eval()
        with torch.no_grad():  # put the median logit of the first frame on the threshold, so the mask keeps about half the rays
            net.outc.conv.bias -= net(nvs.raydrop_features(K, gts[0]["lidar_pose"], H, W)).median()
        net.pack()
        nvs.set_raydrop(net)
    else:
        nvs = _pcgen_nvs(kind, H, W)
    try:
        means, ev = nvs.evaluate(gts, raydrop=raydrop)
        acc, rows = ev.rows()
        assert set(means) == set(nvs_eval.METRICS) and all(isinstance(v, float) for v in means.values())
        per_frame, preds = [], []
        for k, gt in enumerate(gts):
            predict = nvs.predict_frame_with_raydrop if raydrop else nvs.predict_frame
            pd = predict(gt["lidar_K"], gt["lidar_pose"], H, W)
            before = [a.copy() for a in (gt["pano"], gt["intensities"])]
            m = nvs_mod.eval_points_and_pano(_gt_cloud(gt).cpu().numpy(), pd["local_points"].cpu().numpy(), gt["intensities"],
                                             pd["intensities"].cpu().numpy(), gt["pano"], pd["pano"].cpu().numpy())
            assert np.array_equal(before[0], gt["pano"]) and np.array_equal(before[1], gt["intensities"])  # inputs untouched
            assert all(m[key] == rows[k, _slot(key)] for key in m), (k, m, rows[k])
            per_frame.append(m)
            preds.append(pd)
    finally:
        if kind.startswith("mesh"):
            nvs.set_raydrop(None)
    for key in means:
        total = 0.0
        for m in per_frame:
            total += m[key]
        assert means[key] == total / len(gts) and math.isfinite(means[key])
    want = ref.evaluate(gts[0]["pano"], preds[0]["pano"].cpu().numpy(), gts[0]["intensities"], preds[0]["intensities"].cpu().numpy())
    assert rows[0, _slot("depth_a1")] == want["depth_a1"] and rows[0, _slot("n")] == H * W and 0 < means["depth_a1"] <= 1
    kept = int((preds[0]["pano"] != 0).sum())
    assert means["chamfer"] > 0 and 0 < kept and (kept < H * W or not raydrop)  # the ray-drop models drop some and keep some
    text = ev.report()
    lines = text.splitlines()
    assert lines[0] == "Mean metrics:" and [ln.split(":")[0][2:] for ln in lines[1:]] == sorted(means)
    assert lines[1] == f"- chamfer: {means['chamfer']:.4f}" and text in capsys.readouterr().out


def test_nerf_mvl_crop_bad_frames_and_refusals():
    from lidarnerf.nvs import NVSFrameEvaluator
    H, W = 23, 37
    gt, pd, gi, pi = (torch.from_numpy(a).cuda() for a in _random_frame(H, W, 5))
    window = _mask(H, W, 3, 5, 16, 25).astype(bool)
    ev = NVSFrameEvaluator(H, W, K, nerf_mvl=True, max_frames=2)
    ev.update({"pano": gt, "intensities": gi, "pano_mask": window}, {"pano": pd, "intensities": pi})
    ev.update({"pano": gt.cpu().numpy(), "intensities": gi.cpu().numpy(), "pano_mask": torch.from_numpy(window).cuda()},
              {"pano": pd.cpu().numpy(), "intensities": pi.cpu().numpy()})  # NumPy arrays are moved
    acc, rows = ev.rows()
    assert np.array_equal(rows[0], rows[1]) and tuple(rows[0, _slot("crop_r0"):_slot("n") + 1]) == (3, 5, 16, 25, 400)
    want = ref.evaluate(gt.cpu().numpy(), pd.cpu().numpy(), gi.cpu().numpy(), pi.cpu().numpy(), window)
    assert abs(rows[0, _slot("intensity_mae")] - want["intensity_mae"]) <= 402 * 2.0 ** -52 * want["intensity_mae"]
    assert rows[0, _slot("depth_a2")] == want["depth_a2"] and want["intensity_mae"] > 20
    m = ev.measure()
    assert m["depth_a2"] == want["depth_a2"] and m["chamfer"] == rows[0, _slot("chamfer")]
    ell = window.copy()
    ell[3:10, 5:20] = False
    ev.update({"pano": gt, "intensities": gi, "pano_mask": ell}, {"pano": pd, "intensities": pi})  # (beyond the history)
    with pytest.raises(RuntimeError, match=r"1 of 3 frames cannot be averaged; a frame beyond the 2 kept"):
        ev.measure()
    ev.clear()
    ev.update({"pano": gt, "intensities": gi, "pano_mask": ell}, {"pano": pd, "intensities": pi})
    with pytest.raises(RuntimeError, match=r"1 of 1 frames cannot be averaged; frame 0: its 295 masked pixels do not fill their 16 x 25"):
        ev.measure()
    ev.clear()
    ev.update({"pano": gt, "intensities": gi, "pano_mask": np.zeros((H, W), bool)}, {"pano": pd, "intensities": pi})
    with pytest.raises(RuntimeError, match="its mask is empty"):
        ev.measure()
    ev.clear()
    ev.update({"pano": gt, "intensities": gi, "pano_mask": window}, {"pano": pd * 0, "intensities": pi})
    with pytest.raises(RuntimeError, match="chamfer = nan"):
        ev.measure()
    with pytest.raises(KeyError, match="pano_mask"):
        ev.update({"pano": gt, "intensities": gi}, {"pano": pd, "intensities": pi})
    with pytest.raises(ValueError, match=r"\[23, 37\]"):
        ev.update({"pano": gt[:, :-1], "intensities": gi, "pano_mask": window}, {"pano": pd, "intensities": pi})
    with pytest.raises(ValueError, match="holds 900 points"):
        ev.update({"pano": gt, "intensities": gi, "pano_mask": window},
                  {"pano": pd, "intensities": pi, "local_points": torch.zeros(900, 3, device="cuda")})
    with pytest.raises(ValueError, match="intrinsics"):
        NVSFrameEvaluator(H, W, None).update({"pano": gt, "intensities": gi}, {"pano": pd, "intensities": pi})


def test_update_reads_nothing_back_and_a_captured_update_replays_to_the_same_bits():
    from lidarnerf.nvs import NVSFrameEvaluator
    H, W = 66, 1030
    frames = [tuple(torch.from_numpy(a).cuda() for a in _random_frame(H, W, s)) for s in (41, 42)]
    as_dicts = lambda f: ({"pano": f[0], "intensities": f[2]}, {"pano": f[1], "intensities": f[3]})
    ev = NVSFrameEvaluator(H, W, K, max_frames=4)
    ev.update(*as_dicts(frames[0]))  # (allocations warmed)
    ev.clear()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f in frames:
            ev.update(*as_dicts(f))
        ev.update({"pano": frames[0][0], "intensities": frames[0][2]},
                  {"pano": frames[0][1], "intensities": frames[0][3], "local_points": ev.points.clouds[1, :5000, :3].clone()})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    eager = ev.state.clone()
    assert int(eager[0, _slot("frames")]) == 3 and bool(torch.isfinite(eager[:4]).all())
    assert float(eager[3, _slot("chamfer")]) != float(eager[1, _slot("chamfer")])  # the explicit cloud was used
    held = [t.clone() for t in frames[0]]
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(*as_dicts(held))
    ev.clear()
    for f in frames:
        for dst, src in zip(held, f):
            dst.copy_(src)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(ev.state[1:3]), _bits(eager[1:3]))
    assert torch.equal(_bits(ev.state[0]), _bits(eager[1] + eager[2]))


# ------------------------------------------------------------------------------------------------------ the trained field
RENDER = dict(num_steps=768, upsample_steps=64)


def _trainer(graph=False, **kw):
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph, render_kwargs=RENDER, **kw)
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, 1024, 0, dev, (1, 1), "analytic") for s in range(8)]
    return tr, model, batches, poses


def _field_frames(poses, H, W):
    rng = np.random.default_rng(3)
    return [{"pano": rng.uniform(1, 60, (H, W)).astype(F), "intensities": rng.random((H, W), F), "lidar_K": K,
             "lidar_pose": poses[k], "lidar_H": H, "lidar_W": W} for k in (0, 1)]


def test_field_nvs_returns_test_steps_images():
    import bench
    from lidarnerf.dataset.rays import get_lidar_rays
    from lidarnerf.nvs import FieldNVS, evaluate_nvs
    # alpha_r = 0: test_step leaves its images unmasked, so a field of three steps (which predicts no return yet) has depths
    tr, model, batches, poses = _trainer(ema_decay=0.95, ema_interval=1, alpha_r=0.0)
    for b in batches[:3]:
        tr.step(*b)
    H, W = 8, 128
    field = FieldNVS(tr, bench.SCALE)
    got = field.predict_frame_with_raydrop(K, poses[2], H, W)
    assert model.training and set(got) == {"pano", "intensities"} and got["pano"].shape == (H, W)
    assert float(got["pano"].min()) > 0 and bool(torch.isfinite(got["intensities"]).all())
    data = field.rays(K, poses[2], H, W)
    rays = get_lidar_rays(poses[2:3], K, H, W, -1)
    assert torch.allclose(data["rays_d_lidar"], rays["rays_d"].reshape(1, H * W, 3), atol=1e-6)
    model.eval()
    with tr.ema_weights():
        _, want_i, want_d = tr.test_step(data)
    raw_d = tr.test_step(data)[2]
    model.train()
    assert torch.equal(_bits(got["pano"]), _bits(want_d[0] / bench.SCALE)) and torch.equal(_bits(got["intensities"]), _bits(want_i[0]))
    plain = FieldNVS(tr, bench.SCALE, ema=False).predict_frame_with_raydrop(K, poses[2], H, W)
    assert torch.equal(_bits(plain["pano"]), _bits(raw_d[0] / bench.SCALE)) and not torch.equal(plain["pano"], got["pano"])
    means, ev = evaluate_nvs(field, _field_frames(poses, H, W))
    assert set(means) == {"depth_rmse", "depth_a1", "depth_a2", "depth_a3", "depth_ssim", "intensity_mae", "chamfer", "f_score"}
    assert all(math.isfinite(v) for v in means.values()) and ev.rows()[1].shape[0] == 2


@pytest.mark.parametrize("graph", [False, True])
def test_training_does_not_notice_an_evaluation(graph):
    """Eight steps from one seed with an evaluation of the field after the fourth against eight without: the table, its fp16
    copy, the Adam moments, the optimizer scalars, every MLP matrix and all losses bit for bit."""
    import bench
    from lidarnerf.nvs import FieldNVS, evaluate_nvs

    def run(evaluate):
        tr, model, batches, poses = _trainer(graph=graph, ema_decay=0.95, ema_interval=1, alpha_r=0.0)
        torch.manual_seed(11)
        losses = []
        for s in range(8):
            losses.append(tr.step(*batches[s]).detach().clone())
            if evaluate and s == 3:
                means, _ = evaluate_nvs(FieldNVS(tr, bench.SCALE), _field_frames(poses, 8, 128))
                assert model.training and math.isfinite(means["depth_rmse"])
        torch.cuda.synchronize()
        state = [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()]
        return state + [p.detach().clone() for p in tr.small] + [torch.stack(losses)]

    a, b = run(False), run(True)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), i
    assert torch.isfinite(a[-1]).all()
