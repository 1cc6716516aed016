"""The fused points meter on the device (csrc/eval_points.hip, metrics.FramePointsEvaluator, LidarTrainer.evaluate(
fused_points=True) / nerf.evaluate.evaluate(fused_points=True)): the nearest-neighbour search bit for bit against the C oracle, the projected clouds bit for bit against
convert.pano_to_lidar, the frame's row against the NumPy restatement (tests/eval_points_ref.py) and the untouched
PointsMeter, accumulation, frames without a chamfer distance, run-to-run and captured-graph bit identity, and the trainer.

Bounds: distances, indices, clouds and counts exact; chamfer distance and the two means 1e-12 relative against the
restatement on the same clouds (the same float32 distances summed in double, in another order); F-score, precision and recall exact (ratios of
the same integer counts in double); 1e-5 relative against PointsMeter, which averages in float32; clouds against the NumPy
back-projection rtol = atol = 2e-6 (tests/test_convert_gpu.py's bound for sinf / cosf last-bit differences)."""
import os

import numpy as np
import pytest
import torch

import eval_points_ref as ref
from oracle import c_oracle

pytestmark = pytest.mark.gpu
SCALE, K = 0.0107848535, (2.0, 26.9)
TILE_Q = 1024  # query points per workgroup (kTileQ of csrc/eval_points.hip)


def _rel(got, want):
    return abs(got - want) / abs(want)


def _nn(a, b, cap):
    """Both directions through lnh_eval_points_nn with the clouds written straight into [cap, 4] buffers; rows >= count (and
    the fourth column) hold NaN: a read of them would poison a distance."""
    from lidarnerf import _hip
    n, m = len(a), len(b)
    clouds = torch.full((2, cap, 4), float("nan"), device="cuda")
    clouds[0, :n, :3] = torch.from_numpy(a).cuda()
    clouds[1, :m, :3] = torch.from_numpy(b).cuda()
    counts = torch.tensor([n, m, 0, 0], dtype=torch.int32, device="cuda")
    nbytes = int(_hip.lib().lnh_eval_points_workspace_bytes(1, cap))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    dist = torch.full((2, cap), -1.0, device="cuda")
    idx = torch.full((2, cap), -1, dtype=torch.int32, device="cuda")
    _hip.call("lnh_eval_points_nn", clouds[0].data_ptr(), clouds[1].data_ptr(), counts.data_ptr(), cap, ws.data_ptr(),
              ws.numel() * 8, dist[0].data_ptr(), idx[0].data_ptr(), dist[1].data_ptr(), idx[1].data_ptr())
    d, i = dist.cpu().numpy(), idx.cpu().numpy()
    assert (d[0, n:] == -1).all() and (d[1, m:] == -1).all() and (i[0, n:] == -1).all() and (i[1, m:] == -1).all()
    return d[0, :n], i[0, :n], d[1, :m], i[1, :m]


# (n, m, capacity): the three shapes of test_chamfer_nn_bit_exact with a little surplus capacity; one query above a multiple
# of the query tile against 40 000 targets in buffers of a full 66 x 1030 frame — 16 slices of 2560 targets there, so slice
# boundaries and LDS tile boundaries (1024) both fall inside the cloud
@pytest.mark.parametrize("n,m,cap", [(1, 1, 1), (1, 1, 40), (257, 1025, 1100), (3000, 2100, 3001),
                                     (TILE_Q + 1, 40000, 66 * 1030)])
def test_nearest_neighbour_bit_exact(n, m, cap):
    rng = np.random.default_rng(n + m)
    a = rng.normal(size=(n, 3)).astype(np.float32)
    b = rng.normal(size=(m, 3)).astype(np.float32)
    if m > 10:
        b[7] = b[3]            # duplicate target: the first index must win
        a[0] = b[3]            # exact hit
    if m == 40000:
        b[1500] = b[100]       # the same slice, another LDS tile
        b[5000] = b[100]       # another slice
        a[1] = b[100]
        b[30000] = b[3000]     # slices 1 and 11
        a[2] = b[3000] + np.float32(1e-3)
        a[TILE_Q] = b[39999]   # the lone query of the second tile hits the last target
    want_d1, want_i1 = c_oracle.chamfer_nn(a, b)
    want_d2, want_i2 = c_oracle.chamfer_nn(b, a)
    d1, i1, d2, i2 = _nn(a, b, cap)
    assert np.array_equal(i1, want_i1) and np.array_equal(d1, want_d1)
    assert np.array_equal(i2, want_i2) and np.array_equal(d2, want_d2)
    if m > 10:
        assert d1[0] == 0.0 and i1[0] == 3
    if m == 40000:
        assert (d1[1], i1[1]) == (0.0, 100) and i1[2] == 3000 and (d1[TILE_Q], i1[TILE_Q]) == (0.0, 39999)


def _frame(seed, H, W, zero=0.2, mvl=False, scale=SCALE):
    """A ground-truth frame [H, W, 3] and a predicted depth [H, W] with about `zero` of the depths 0 on each side, built like
    tests/test_metrics_gpu.py::test_meters_match_restatement (2 % noise; a few predicted returns where the truth has none)."""
    rng = np.random.default_rng(seed)
    raydrop = (rng.uniform(size=(H, W)) > zero).astype(np.float32)
    depth = (rng.uniform(2.0, 70.0, (H, W)) * scale).astype(np.float32)
    gt = np.stack([raydrop, rng.uniform(size=(H, W)).astype(np.float32), depth], -1)
    if mvl:
        gt[:, :5, 0] = -1.0
        gt[0, :, 0] = -1.0
    present = gt[..., 0] == 1
    pred = depth * present * rng.normal(1.0, 0.02, (H, W)) + (~present) * (rng.uniform(size=(H, W)) > 0.97) * 5.0 * scale
    pred = pred * (rng.uniform(size=(H, W)) > zero * 0.25)
    return torch.from_numpy(pred.astype(np.float32)).cuda(), torch.from_numpy(gt).cuda()


def _torch_inputs(pred, gt, mvl):
    """What evaluate() hands to PointsMeter.update (nerf/evaluate.py)."""
    gr = gt[..., 0]
    if mvl:
        gr = gr * torch.where(gr == -1, 0, 1)
    return pred, gt[..., 2] * gr


def _evaluator(H, W, **kw):
    from lidarnerf import metrics
    return metrics.FramePointsEvaluator(H, W, SCALE, K, **kw)


def _check_clouds(ev, pred, gt, mvl):
    from lidarnerf import convert
    ev.update(pred, gt)
    counts = [int(c) for c in ev.counts[:2].cpu()]
    p, g = _torch_inputs(pred, gt, mvl)
    want = [convert.pano_to_lidar(x / SCALE, K) for x in (p, g)]
    for c in range(2):
        got = ev.clouds[c, :counts[c]]
        assert counts[c] == want[c].shape[0], (c, counts, want[c].shape)
        assert torch.equal(got[:, :3], want[c]) and not got[:, 3].any()
    assert torch.equal(ev.cloud(), want[0])
    rp, rg = ref.clouds(pred.cpu().numpy(), gt.cpu().numpy(), SCALE, K, mvl)
    for c, r in enumerate((rp, rg)):
        assert r.shape == (counts[c], 3)
        np.testing.assert_allclose(ev.clouds[c, :counts[c], :3].cpu().numpy(), r, rtol=2e-6, atol=2e-6)
    return counts


@pytest.mark.parametrize("H,W", [(8, 70), (16, 130)])
@pytest.mark.parametrize("mvl", [False, True], ids=["kitti", "nerf_mvl"])
def test_projected_clouds_equal_pano_to_lidar(H, W, mvl):
    pred, gt = _frame(H + W, H, W, mvl=mvl)
    assert not mvl or (gt[..., 0] == -1).any()
    ev = _evaluator(H, W, nerf_mvl=mvl)
    counts = _check_clouds(ev, pred, gt, mvl)
    assert 0.6 * H * W < counts[0] < 0.95 * H * W and 0.6 * H * W < counts[1] < 0.95 * H * W
    # every pixel valid
    full_gt = gt.clone()
    full_gt[..., 0] = 1.0
    full_pred = full_gt[..., 2] * 1.01
    assert list(_check_clouds(ev, full_pred, full_gt, mvl)) == [H * W, H * W]
    # the last pixel is the only valid one
    one_gt, one_pred = full_gt.clone(), torch.zeros_like(full_pred)
    one_gt[..., 0] = 0.0
    one_gt[-1, -1, 0] = 1.0
    one_pred[-1, -1] = full_pred[-1, -1]
    assert list(_check_clouds(ev, one_pred, one_gt, mvl)) == [1, 1]
    ev.clear()


def _ref_row(pred, gt, mvl=False):
    """The restatement's row on the clouds convert.pano_to_lidar gives (the fused clouds are held to those bit for bit
    above): the same float32 distances, so the means agree to fp64 summation order.  NumPy's own back-projection differs from
    the device's in the last bit of sinf / cosf, which moves every distance: ref.frame_row is compared more loosely."""
    from lidarnerf import convert
    a, b = (convert.pano_to_lidar(x / SCALE, K).contiguous().cpu().numpy() for x in _torch_inputs(pred, gt, mvl))
    return ref.row_of_clouds(a, b)


def _check_row(row, want):
    for name in ("chamfer", "mean_pred", "mean_gt"):
        print(name, row[name], want[name], _rel(row[name], want[name]))
        assert _rel(row[name], want[name]) <= 1e-12
    for name in ("fscore", "precision", "recall", "count_pred", "count_gt", "frames", "bad"):
        print(name, row[name], want[name])
        assert row[name] == want[name]


def test_whole_row_against_the_restatement_and_the_points_meter():
    from lidarnerf import _hip, metrics
    H, W = 16, 130
    pred, gt = _frame(3, H, W)
    ev = _evaluator(H, W)
    ev.update(pred, gt)
    acc, rows = ev.rows()
    row = dict(zip(_hip.PTS_SLOT_NAMES, rows[0]))
    _check_row(row, _ref_row(pred, gt))
    # the restatement from the depth images, NumPy back-projection included: tests/test_metrics_gpu.py:75-76's bounds
    want = ref.frame_row(pred.cpu().numpy(), gt.cpu().numpy(), SCALE, K)
    print("numpy clouds", want)
    assert _rel(row["chamfer"], want["chamfer"]) < 1e-3 and abs(row["fscore"] - want["fscore"]) < 2e-3
    assert (row["count_pred"], row["count_gt"]) == (want["count_pred"], want["count_gt"])
    assert 0.0 < row["fscore"] < 1.0 and np.array_equal(acc, rows[0])
    pm = metrics.PointsMeter(SCALE, K)
    p, g = _torch_inputs(pred, gt, False)
    pm.update(p[None], g[None])
    got, old = ev.measure(), pm.measure()
    print("fused", got, "PointsMeter", old)
    assert got.shape == (2,) and _rel(got[0], old[0]) <= 1e-5 and _rel(got[1], old[1]) <= 1e-5
    assert ev.report() == f"CD f-score = {got}" and ev.report().startswith("CD f-score = [")


def test_full_size_frame_against_the_points_meter_and_chamfer_nn():
    from lidarnerf import _hip, convert, metrics
    H, W = 66, 1030
    pred, gt = _frame(9, H, W)
    ev = _evaluator(H, W)
    ev.update(pred, gt)
    n, m = (int(c) for c in ev.counts[:2])
    p, g = _torch_inputs(pred, gt, False)
    a, b = (convert.pano_to_lidar(x / SCALE, K).contiguous() for x in (p, g))
    assert (n, m) == (a.shape[0], b.shape[0]) and torch.equal(ev.clouds[0, :n, :3], a) and torch.equal(ev.clouds[1, :m, :3], b)
    d1, d2, i1, i2 = metrics.chamfer_3DDist()(a[None], b[None])
    assert torch.equal(ev.dist[0, :n], d1[0]) and torch.equal(ev.dist[1, :m], d2[0])
    assert torch.equal(ev.idx[0, :n], i1[0]) and torch.equal(ev.idx[1, :m], i2[0])
    pm = metrics.PointsMeter(SCALE, K)
    pm.update(p[None], g[None])
    got, old = ev.measure(), pm.measure()
    print("fused", got, "PointsMeter", old)
    assert _rel(got[0], old[0]) <= 1e-5 and _rel(got[1], old[1]) <= 1e-5
    row = dict(zip(_hip.PTS_SLOT_NAMES, ev.rows()[1][0]))
    assert _rel(row["mean_pred"], float(d1[0].double().mean())) <= 1e-12 and _rel(row["mean_gt"], float(d2[0].double().mean())) <= 1e-12
    assert row["precision"] == float((d1[0] < 0.05).sum()) / n and row["recall"] == float((d2[0] < 0.05).sum()) / m


def test_accumulation_and_history():
    from lidarnerf import _hip
    H, W = 16, 130
    frames = [_frame(20 + k, H, W, zero=z) for k, z in enumerate((0.1, 0.3, 0.5))]
    want = [_ref_row(p, g) for p, g in frames]
    assert len({w["count_gt"] for w in want}) == 3
    for max_frames in (8, 2, 0):
        ev = _evaluator(H, W, max_frames=max_frames)
        for p, g in frames:
            ev.update(p, g)
        acc, rows = ev.rows()
        assert rows.shape == (min(3, max_frames), _hip.PTS_SLOTS)
        for k in range(rows.shape[0]):
            _check_row(dict(zip(_hip.PTS_SLOT_NAMES, rows[k])), want[k])
        got = ev.measure()
        assert _rel(got[0], np.mean([w["chamfer"] for w in want])) <= 1e-12
        assert _rel(got[1], np.mean([w["fscore"] for w in want])) <= 1e-12
        assert acc[_hip.PTS_SLOT_NAMES.index("frames")] == 3 and acc[_hip.PTS_SLOT_NAMES.index("bad")] == 0
        if max_frames == 8:
            assert np.array_equal(acc, rows[0] + rows[1] + rows[2])  # (added in frame order)


def test_a_frame_with_an_empty_cloud_is_counted_and_refused():
    H, W = 16, 130
    pred, gt = _frame(4, H, W)
    ev = _evaluator(H, W, max_frames=2)
    ev.update(pred, gt)
    good = ev.measure()
    ev.update(torch.zeros_like(pred), gt)                 # no predicted return at all
    with pytest.raises(RuntimeError, match="1 of 2 frames have no chamfer distance; frame 1: 0 predicted and"):
        ev.measure()
    assert ev.cloud().shape == (0, 3)
    none = gt.clone()
    none[..., 0] = 0.0
    ev.update(pred, none)                                 # no ground-truth return (the third frame: beyond the history)
    with pytest.raises(RuntimeError, match="2 of 3 frames"):
        ev.measure()
    ev.clear()
    ev.update(pred, none)
    ev.update(pred, gt)
    ev.clear()
    ev.update(pred, gt)
    ev.update(pred, gt)
    ev.update(torch.zeros_like(pred), none)               # both clouds empty, beyond the two rows kept
    with pytest.raises(RuntimeError, match="1 of 3 frames .* beyond the 2 kept"):
        ev.measure()
    ev.clear()
    ev.update(pred, gt)
    torch.cuda.synchronize()
    assert np.array_equal(ev.measure(), good)


def test_two_runs_and_a_captured_graph_give_identical_rows():
    H, W = 16, 130
    frames = [_frame(30 + k, H, W, zero=z) for k, z in enumerate((0.2, 0.6, 0.05))]

    def eager():
        ev = _evaluator(H, W, max_frames=8)
        for p, g in frames:
            ev.update(p, g)
        return ev.state.clone()

    s0, s1 = eager(), eager()
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64))
    assert int(s0[0, 8]) == 3 and torch.isfinite(s0[:4]).all() and len({float(v) for v in s0[1:4, 6]}) == 3

    ev = _evaluator(H, W, max_frames=8)
    pred_s, gt_s = (t.clone() for t in frames[0])
    ev.update(pred_s, gt_s)  # (buffers exist before the capture)
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (a synchronising call inside update() would fail the capture)
        ev.update(pred_s, gt_s)
    ev.clear()
    for p, g in frames:
        pred_s.copy_(p), gt_s.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ev.state.view(torch.int64), s0.view(torch.int64))  # (a count baked in at capture: a wrong row)


def test_trainer_evaluate_with_fused_points(tmp_path):
    import bench
    from test_eval_frame_gpu import _bits, _frame_data, _trainer

    def run(evaluate):
        tr, model, batches = _trainer()
        for b in batches[:3]:
            tr.step(*b)
        results = []
        if evaluate:
            frames = [_frame_data(b) for b in batches[5:7]]
            for fused in (False, True):
                d = os.path.join(tmp_path, "fused" if fused else "meter")
                tr.fused_points = fused  # (the method's parameter list is pinned: the trainer carries the switch)
                results.append(tr.evaluate(frames, points_intrinsics=bench.INTRINSICS, save_dir=d))
            # the keyword of the loop itself, against the attribute route: the same evaluation, bit for bit
            from lidarnerf.nerf import evaluate as loop
            tr.fused_points = False
            again = loop.evaluate(tr, frames, points_intrinsics=bench.INTRINSICS, fused_points=True)
            assert np.array_equal(again["points"], results[1]["points"]) and again["loss"] == results[1]["loss"]
            tr.stats["results"].pop(), tr.stats["valid_loss"].pop()
            assert model.training
        for b in batches[3:5]:
            tr.step(*b)
        torch.cuda.synchronize()
        return tr, _bits(model), results

    tr, with_eval, (old, new) = run(True)
    print("PointsMeter", old["points"], "fused", new["points"])
    assert new["points"].shape == old["points"].shape == (2,) and np.isfinite(new["points"]).all()
    assert _rel(new["points"][0], old["points"][0]) <= 1e-5 and _rel(new["points"][1], old["points"][1]) <= 1e-5
    assert tr.stats["results"] == [float(old["points"][0]), float(new["points"][0])]
    assert tr.stats["valid_loss"] == [old["loss"], new["loss"]] and old["loss"] == new["loss"]
    names = sorted(os.listdir(os.path.join(tmp_path, "meter")))
    assert names == ["ep0000_0001_lidar.npy", "ep0000_0002_lidar.npy"] == sorted(os.listdir(os.path.join(tmp_path, "fused")))
    for name in names:
        a, b = (open(os.path.join(tmp_path, d, name), "rb").read() for d in ("meter", "fused"))
        assert a == b and np.load(os.path.join(tmp_path, "fused", name)).shape[1] == 3
    _, plain, _ = run(False)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, with_eval))
