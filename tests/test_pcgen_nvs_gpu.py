"""The point-cloud baseline on the device (lidarnerf/nvs.py: PointCloudNVS, LidarNVSPCGen of lidarnvs/lidarnvs_pcgen.py): the ray
directions against G16's float64 images of the reference's get_direction, predict_frame against the hand-chained public calls bit
for bit, the ray-drop rows and their filtering, and predict_frame_with_raydrop with the package's own RayDropMLP."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = (2.0, 26.9)
FRAMES = [(6, 16), (66, 1030)]
KEYS = {"pano", "intensities", "points", "point_intensities", "local_points", "local_point_intensities"}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pose():
    a, b = 0.3, -0.05
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = (rz @ rx).astype(np.float32)
    pose[:3, 3] = [11.4, -3.9, 1.2]
    return pose


@functools.lru_cache(maxsize=None)
def _cloud():
    """30000 world-frame points seen from the pose inside (and a little outside) the sensor's field of view, 3 to 90 m away (some
    beyond max_depth), with intensities in [0, 1]."""
    rng = np.random.default_rng(21)
    n = 30000
    az = rng.uniform(-np.pi, np.pi, n)
    el = np.radians(rng.uniform(-27.0, 4.0, n))
    d = rng.uniform(3, 90, n)
    local = np.stack([d * np.cos(el) * np.cos(az), d * np.cos(el) * np.sin(az), d * np.sin(el)], 1)
    pose = _pose().astype(np.float64)
    pts = (local @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    inten = rng.uniform(0, 1, n).astype(np.float32)
    pts.setflags(write=False), inten.setflags(write=False)
    return pts, inten


@functools.lru_cache(maxsize=None)
def _nvs(raycasting):
    from lidarnerf.nvs import PointCloudNVS
    pts, inten = _cloud()
    return PointCloudNVS(pts, inten, raycasting=raycasting)


@functools.lru_cache(maxsize=None)
def _frame(raycasting, H, W):
    return _nvs(raycasting).predict_frame(K, _pose(), H, W)


def test_directions_against_the_reference_in_float64():
    """Within twice NumPy's own fp32 deviation from the float64 image (the rule of test_sampler_gpu.py for get_lidar_rays).  The
    66 x 1030 image is stored as its factors, which the generator asserts to reproduce the reference's image bit for bit."""
    g = np.load(os.path.join(GOLDEN, "g16_raydrop.npz"))
    nvs = _nvs("cp")
    ca, sa, cb, sb = g["dir_ca"], g["dir_sa"], g["dir_cb"], g["dir_sb"]
    large = np.stack([ca[:, None] * cb[None, :], ca[:, None] * sb[None, :], np.broadcast_to(sa[:, None], (66, 1030))], -1)
    for (H, W), want, dev in (((6, 16), g["dir_small"], g["dir_dev_small"]), ((66, 1030), large, g["dir_dev_large"])):
        got = nvs.directions(K, H, W)
        assert got.shape == (H, W, 3) and got.dtype == torch.float32 and got.is_cuda
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"directions {H} x {W}: device deviates by {err:.3g}, NumPy's fp32 by {float(dev):.3g}")
        assert err <= 2 * float(dev)
        assert abs(float(got.norm(dim=-1).max()) - 1) < 1e-6


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("raycasting", ["cp", "fpa"])
def test_predict_frame_equals_the_hand_chained_calls(raycasting, H, W):
    from lidarnerf import convert, nvs as nvs_mod
    pts, inten = _cloud()
    frame = _frame(raycasting, H, W)
    assert set(frame) == KEYS and all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in frame.values())
    dpose = torch.from_numpy(_pose()).cuda()
    local = nvs_mod.world_to_lidar(torch.from_numpy(pts).cuda(), dpose)
    rows = torch.cat([local, torch.from_numpy(inten).cuda()[:, None]], dim=1)
    if raycasting == "cp":
        pano, intensities = convert.lidar_to_pano_with_intensities(rows, H, W, K)
    else:
        pano, intensities = convert.lidar_to_pano_with_intensities_fpa(rows, H, W, K, z_buffer_len=10)
    assert _same(frame["pano"], pano) and _same(frame["intensities"], intensities) and pano.shape == (H, W)
    filled = int((pano != 0).sum())
    assert filled > 0.2 * H * W and float(pano.max()) < 80
    back = convert.pano_to_lidar_with_intensities(pano, intensities, K)
    assert back.shape == (filled, 4)
    assert _same(frame["local_points"], back[:, :3].contiguous()) and _same(frame["local_point_intensities"], back[:, 3].contiguous())
    assert _same(frame["points"], nvs_mod.transform_points(back[:, :3].contiguous(), dpose))
    assert _same(frame["point_intensities"], frame["local_point_intensities"])
    if (H, W) == (6, 16):  # the two ray casters differ where a pixel holds several points (here: hundreds in every pixel)
        other = _frame("fpa" if raycasting == "cp" else "cp", H, W)
        assert bool(torch.equal(other["pano"] != 0, pano != 0)) and not torch.equal(other["pano"], pano)


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("raycasting", ["cp", "fpa"])
def test_without_the_clouds_nothing_synchronises(raycasting, H, W):
    nvs = _nvs(raycasting)
    frame = _frame(raycasting, H, W)
    dpose = torch.from_numpy(_pose()).cuda()
    nvs.predict_frame(K, dpose, H, W, compact=False)  # (allocations warmed)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lean = nvs.predict_frame(K, dpose, H, W, compact=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(lean) == {"pano", "intensities"}
    assert _same(lean["pano"], frame["pano"]) and _same(lean["intensities"], frame["intensities"])


def test_raydrop_rows_and_their_filtering():
    H, W = 6, 16
    nvs = _nvs("cp")
    frame = _frame("cp", H, W)
    rows = nvs.raydrop_rows(K, _pose(), H, W)
    assert rows.shape == (H * W, 5) and rows.dtype == torch.float32
    assert _same(rows[:, :3].contiguous(), nvs.directions(K, H, W).reshape(-1, 3))
    assert _same(rows[:, 3].contiguous(), frame["pano"].reshape(-1)) and _same(rows[:, 4].contiguous(), frame["intensities"].reshape(-1))
    gt = np.full((H, W), 7.5, dtype=np.float32)
    gt[0, :5] = -1.0   # outside the box mask: left out
    gt[2, 3:9] = 0.0   # dropped rays: target 0
    gt[5, 15] = 0.25   # a return: target 1
    for given in (gt, torch.from_numpy(gt).cuda()):
        train = nvs.raydrop_rows(K, _pose(), H, W, gt_pano=given)
        keep = gt.reshape(-1) > -1
        assert train.shape == (H * W - 5, 6) and _same(train[:, :5].contiguous(), rows[torch.from_numpy(keep).cuda()])
        want = np.where(gt.reshape(-1)[keep] == 0, 0.0, 1.0).astype(np.float32)
        assert np.array_equal(train[:, 5].cpu().numpy(), want) and want.sum() == H * W - 5 - 6
    with pytest.raises(ValueError, match="gt_pano"):
        nvs.raydrop_rows(K, _pose(), H, W, gt_pano=gt[:, :-1])


@pytest.mark.parametrize("H,W", FRAMES)
def test_predict_frame_with_the_raydrop_mlp(H, W):
    from lidarnerf import convert, nvs as nvs_mod
    from lidarnerf.nvs import PointCloudNVS
    from lidarnerf.raydrop import RayDropMLP
    pts, inten = _cloud()
    frame = _frame("cp", H, W)
    torch.manual_seed(6)
    model = RayDropMLP(4, 128).cuda()
    rows = _nvs("cp").raydrop_rows(K, _pose(), H, W)
    with torch.no_grad():  # put the median output on the threshold, so the mask keeps about half the rays
        model.output_linear.bias += 0.5 - model(rows).median()
    nvs = PointCloudNVS(pts, inten, raycasting="cp", raydrop=model)
    got = nvs.predict_frame_with_raydrop(K, _pose(), H, W)
    assert set(got) == KEYS
    keep = (model(rows) > 0.5).reshape(H, W)
    assert 0.2 * H * W < int(keep.sum()) < 0.8 * H * W and _same(model.predict_mask(rows).reshape(H, W), keep.float())
    assert _same(got["pano"], frame["pano"] * keep.float()) and _same(got["intensities"], frame["intensities"] * keep.float())
    assert bool(torch.equal(got["pano"] != 0, (frame["pano"] != 0) & keep))
    back = convert.pano_to_lidar_with_intensities(got["pano"], got["intensities"], K)
    assert back.shape[0] == int(((frame["pano"] != 0) & keep).sum())
    assert _same(got["local_points"], back[:, :3].contiguous()) and _same(got["local_point_intensities"], back[:, 3].contiguous())
    dpose = torch.from_numpy(_pose()).cuda()
    assert _same(got["points"], nvs_mod.transform_points(back[:, :3].contiguous(), dpose))
    # a model passed to the call takes precedence; any callable serves
    seen = []

    def keep_all(r):
        seen.append(r)
        return torch.ones(r.shape[0], 1, device=r.device)
    full = nvs.predict_frame_with_raydrop(K, _pose(), H, W, raydrop=keep_all)
    assert _same(seen[0], rows) and _same(full["pano"], frame["pano"]) and _same(full["points"], frame["points"])


def test_an_all_dropped_frame_stays_unmasked_and_a_wrong_shape_is_refused():
    from lidarnerf.nvs import PointCloudNVS
    H, W = 6, 16
    pts, inten = _cloud()
    frame = _frame("fpa", H, W)
    nvs = PointCloudNVS(pts, inten, raycasting="fpa", raydrop=lambda r: torch.full((r.shape[0], 1), -1.0, device=r.device))
    got = nvs.predict_frame_with_raydrop(K, _pose(), H, W)
    for k in frame:
        assert _same(got[k], frame[k]), k
    at_threshold = nvs.predict_frame_with_raydrop(K, _pose(), H, W, raydrop=lambda r: torch.full((r.shape[0], 1), 0.5, device=r.device))
    assert _same(at_threshold["pano"], frame["pano"])  # 0.5 is not > 0.5: all dropped again
    one = torch.zeros(H * W, 1, device="cuda")
    one[int((frame["pano"].reshape(-1) != 0).nonzero()[0])] = 1.0
    single = nvs.predict_frame_with_raydrop(K, _pose(), H, W, raydrop=lambda r: one)
    assert int((single["pano"] != 0).sum()) == 1 and single["points"].shape == (1, 3)
    for bad in (lambda r: torch.zeros(r.shape[0], device=r.device), lambda r: torch.zeros(1, 1, H, W, device=r.device),
                lambda r: torch.zeros(r.shape[0] + 1, 1, device=r.device), lambda r: None):
        with pytest.raises(ValueError, match=r"must return \[96, 1\]"):
            nvs.predict_frame_with_raydrop(K, _pose(), H, W, raydrop=bad)
    with pytest.raises(RuntimeError, match="no ray-drop model"):
        PointCloudNVS(pts, inten).predict_frame_with_raydrop(K, _pose(), H, W)


def test_fit_concatenates_and_refusals():
    from lidarnerf.nvs import PointCloudNVS
    pts, inten = _cloud()
    frames = [{"points": pts[:10000], "point_intensities": inten[:10000]},
              {"points": torch.from_numpy(pts[10000:]).cuda(), "point_intensities": torch.from_numpy(inten[10000:])}]
    nvs = PointCloudNVS(raycasting="fpa", z_buffer_len=10)
    with pytest.raises(RuntimeError, match="no cloud yet"):
        nvs.predict_frame(K, _pose(), 6, 16)
    assert nvs.fit(frames) is nvs and nvs.points.shape == (30000, 3) and nvs.points.is_cuda
    assert np.array_equal(nvs.points.cpu().numpy(), pts) and np.array_equal(nvs.point_intensities.cpu().numpy(), inten)
    got, want = nvs.predict_frame(K, _pose(), 6, 16), _frame("fpa", 6, 16)
    for k in want:
        assert _same(got[k], want[k]), k
    with pytest.raises(ValueError, match="'cp' or 'fpa'"):
        PointCloudNVS(pts, inten, raycasting="mesh")
    with pytest.raises(ValueError, match="must be 30000 floats"):
        PointCloudNVS(pts, inten[:-1])
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        PointCloudNVS(pts[:, :2], inten)
    with pytest.raises(ValueError, match=r"\[4, 4\]"):
        nvs.predict_frame(K, np.eye(3), 6, 16)
