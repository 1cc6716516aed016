"""predict_frame of the mesh NVS on the device (lidarnerf/nvs.py: MeshNVS) against the composition of its public pieces — the
scene's intersect_lidar, the NumPy restatement of the nearest-neighbour contract (tests/knn_ref.py) on the hit points, and
convert.lidar_to_pano_with_intensities on the compacted cloud.  Every comparison with a reference is bit for bit: no tolerance is
used for any of them."""
import functools
import math

import numpy as np
import pytest
import torch

import knn_ref as kr
import marching_cubes_ref as mc

pytestmark = pytest.mark.gpu
K = (2.0, 26.9)
FRAMES = [(6, 16), (66, 1030)]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _pose():
    a, b = 0.3, -0.2
    rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = (rz @ rx).astype(np.float32)
    pose[:3, 3] = [11.4, 13.9, 12.2]
    return pose


@functools.lru_cache(maxsize=None)
def _setup():
    """The 24^3 sphere mesh, a 3000-point cloud sampled near it with random intensities, the NVS object (k = 5)."""
    from lidarnerf.nvs import MeshNVS
    from lidarnerf.raycast import RaycastingScene
    vol, iso = mc.sphere_volume((24, 24, 24), 8.3)
    v, t, _ = mc.marching_cubes(vol, iso)
    rng = np.random.default_rng(17)
    cloud = (v[rng.integers(0, len(v), 3000)] + rng.normal(0, 0.15, (3000, 3))).astype(np.float32)
    inten = rng.uniform(0, 1, 3000).astype(np.float32)
    scene = RaycastingScene(v, t)
    nvs = MeshNVS(scene, cloud, inten)
    assert nvs.k == 5 and nvs.index.N == 3000 and nvs.points.is_cuda and nvs.point_intensities.dtype == torch.float32
    cloud.setflags(write=False), inten.setflags(write=False)
    return scene, nvs, cloud, inten


@functools.lru_cache(maxsize=None)
def _frame(H, W):
    """predict_frame of the frame and the restatement's intensities of its hit points: computed once, shared."""
    scene, nvs, cloud, inten = _setup()
    frame = nvs.predict_frame(K, _pose(), H, W)
    hit = scene.intersect_lidar(K, _pose(), H, W)
    masks = hit["masks"].cpu().numpy()
    idx, _ = kr.brute_force(cloud, hit["points"].cpu().numpy()[masks], 5)
    want_inten = kr.mean_of(inten, idx)
    want_inten.setflags(write=False)
    return frame, hit, masks, want_inten


@pytest.mark.parametrize("H,W", FRAMES)
def test_predict_frame_equals_the_composition_of_its_pieces(H, W):
    from lidarnerf import convert, nvs as nvs_mod
    scene, nvs, cloud, inten = _setup()
    frame, hit, masks, want_inten = _frame(H, W)
    assert set(frame) == {"pano", "intensities", "hit_dict", "points", "point_intensities", "local_points", "local_point_intensities"}
    assert all(torch.is_tensor(x) and x.is_cuda for k, x in frame.items() if k != "hit_dict")
    for k in ("masks", "depths", "points", "normals"):
        assert _same(frame["hit_dict"][k], hit[k]), k
    n_hit = int(masks.sum())
    assert n_hit == H * W  # the sensor sits inside the closed surface (misses: the quad below)
    dmask = hit["masks"]
    # the clouds of the hit points
    assert _same(frame["points"], hit["points"][dmask])
    local = nvs_mod.world_to_lidar(hit["points"], torch.from_numpy(_pose()).cuda())
    assert _same(frame["local_points"], local[dmask])
    back = nvs_mod.transform_points(frame["local_points"], torch.from_numpy(_pose()).cuda())
    # (a sanity check of the inverse pose, not a comparison with a reference: coordinates below 32, about eight roundings of at
    # most ulp(32) / 2 = 1.9e-6 each on the way there and back)
    assert float((back - frame["points"]).abs().max()) < 1e-4
    # the intensities: the restatement's k nearest neighbours, fp64 rank-order mean
    assert np.array_equal(frame["point_intensities"].cpu().numpy().view(np.uint32), want_inten.view(np.uint32))
    assert _same(frame["local_point_intensities"], frame["point_intensities"])
    assert 0 < float(frame["point_intensities"].min()) and float(frame["point_intensities"].max()) < 1
    # the images: the closest-point projection of the COMPACTED cloud
    rows = torch.cat([frame["local_points"], torch.from_numpy(want_inten).cuda()[:, None]], dim=1)
    pano, intensities = convert.lidar_to_pano_with_intensities(rows, H, W, K)
    assert _same(frame["pano"], pano) and _same(frame["intensities"], intensities)
    assert frame["pano"].shape == (H, W) and bool(torch.equal(frame["pano"] != 0, pano != 0))
    filled = int((frame["pano"] != 0).sum())
    print(f"{H} x {W}: {n_hit} hits fill {filled} pixels")
    assert filled >= 0.9 * H * W and not bool(((frame["intensities"] != 0) & (frame["pano"] == 0)).any())


def test_pano_is_empty_exactly_where_nothing_projects():
    """A frame that also misses: a quad seen from above."""
    from lidarnerf import convert
    from lidarnerf.nvs import MeshNVS
    from lidarnerf.raycast import RaycastingScene
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32) * np.float32(4.0)
    scene = RaycastingScene(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    rng = np.random.default_rng(4)
    cloud = np.concatenate([rng.uniform(0, 4, (500, 2)), np.zeros((500, 1))], 1).astype(np.float32)
    inten = rng.uniform(0.2, 1, 500).astype(np.float32)
    nvs = MeshNVS(scene, cloud, inten, intensity_interpolate_k=9)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = [2, 2, 3]
    KQ, H, W = (80.0, 160.0), 8, 32
    frame = nvs.predict_frame(KQ, pose, H, W)
    masks = frame["hit_dict"]["masks"]
    n_hit = int(masks.sum())
    assert 0 < n_hit < H * W and frame["points"].shape == (n_hit, 3) and frame["point_intensities"].shape == (n_hit,)
    idx, _ = kr.brute_force(cloud, frame["points"].cpu().numpy(), 9)
    want = kr.mean_of(inten, idx)
    assert np.array_equal(frame["point_intensities"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    rows = torch.cat([frame["local_points"], frame["point_intensities"][:, None]], dim=1)
    pano, intensities = convert.lidar_to_pano_with_intensities(rows, H, W, KQ)
    assert _same(frame["pano"], pano) and _same(frame["intensities"], intensities)
    filled = frame["pano"] != 0
    assert 0 < int(filled.sum()) <= n_hit and bool(torch.equal(filled, frame["intensities"] != 0))
    # a ray's own hit lands in the ray's own pixel or next to it: no pixel is filled far from every hit
    near = torch.nn.functional.max_pool2d(masks.reshape(1, 1, H, W).float(), 3, 1, 1).bool().reshape(H, W)
    assert not bool((filled & ~near).any())


@pytest.mark.parametrize("H,W", FRAMES)
def test_without_the_clouds_nothing_synchronises(H, W):
    scene, nvs, cloud, inten = _setup()
    frame, *_ = _frame(H, W)
    dpose = torch.from_numpy(_pose()).cuda()
    nvs.predict_frame(K, dpose, H, W, compact=False)  # (allocations warmed)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lean = nvs.predict_frame(K, dpose, H, W, compact=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(lean) == {"pano", "intensities", "hit_dict"}
    assert _same(lean["pano"], frame["pano"]) and _same(lean["intensities"], frame["intensities"])


@pytest.mark.parametrize("H,W", FRAMES)
def test_raydrop_features_carry_the_intensity_image(H, W):
    scene, nvs, cloud, inten = _setup()
    frame, *_ = _frame(H, W)
    img = nvs.raydrop_features(K, _pose(), H, W)
    plain = scene.raydrop_features(K, _pose(), H, W)
    assert img.shape == (1, 10, H, W) and img.dtype == torch.float32 and img.is_cuda
    assert _same(img[0, 6], frame["intensities"]) and bool(frame["intensities"].any()) and not bool(plain[0, 6].any())
    for c in (0, 1, 2, 3, 4, 5, 7, 8, 9):
        assert _same(img[0, c], plain[0, c]), c


@pytest.mark.parametrize("H,W", FRAMES)
def test_predict_frame_with_raydrop_masks_what_the_model_drops(H, W):
    from lidarnerf import convert
    scene, nvs, cloud, inten = _setup()
    frame, *_ = _frame(H, W)
    seen = []

    def constant(value):
        def model(images):
            seen.append(images)
            return torch.full((1, 1, H, W), value, device=images.device)
        return model

    keep = nvs.predict_frame_with_raydrop(K, _pose(), H, W, constant(2.5))
    assert seen[0].shape == (1, 10, H, W) and _same(seen[0], nvs.raydrop_features(K, _pose(), H, W))
    assert set(keep) == {"pano", "intensities", "hit_dict", "points", "point_intensities", "local_points", "local_point_intensities"}
    assert _same(keep["pano"], frame["pano"]) and _same(keep["intensities"], frame["intensities"])
    n = int((frame["pano"] != 0).sum())
    assert keep["points"].shape == (n, 3) and keep["local_points"].shape == (n, 3) and keep["point_intensities"].shape == (n,)
    want = convert.pano_to_lidar_with_intensities(frame["pano"], frame["intensities"], K)
    assert _same(keep["local_points"], want[:, :3].contiguous()) and _same(keep["local_point_intensities"], want[:, 3].contiguous())
    assert _same(keep["point_intensities"], keep["local_point_intensities"])
    # the world-frame cloud lies where the hit points lie: within a pixel's width of the sphere's surface
    centre = torch.tensor([(24 - 1) / 2 + 0.13 * (a + 1) for a in range(3)], device="cuda")
    assert float(((keep["points"] - centre).norm(dim=1) - 8.3).abs().max()) <= math.sqrt(3.0)
    drop = nvs.predict_frame_with_raydrop(K, _pose(), H, W, constant(-2.5))
    assert not bool(drop["pano"].any()) and not bool(drop["intensities"].any())
    assert drop["points"].shape == (0, 3) and drop["local_points"].shape == (0, 3) and drop["point_intensities"].shape == (0,)
    zero = nvs.predict_frame_with_raydrop(K, _pose(), H, W, constant(0.0))  # sigmoid(0) = 0.5 is not > 0.5
    assert not bool(zero["pano"].any())
    board = ((torch.arange(H, device="cuda")[:, None] + torch.arange(W, device="cuda")[None, :]) % 2).bool()
    half = nvs.predict_frame_with_raydrop(K, _pose(), H, W, lambda images: torch.where(board, 1.0, -1.0).reshape(1, 1, H, W))
    assert bool(torch.equal(half["pano"] != 0, (frame["pano"] != 0) & board))
    assert _same(half["pano"][board], frame["pano"][board]) and _same(half["intensities"][board], frame["intensities"][board])
    assert half["points"].shape[0] == int(((frame["pano"] != 0) & board).sum())
    with pytest.raises(ValueError, match="logits"):
        nvs.predict_frame_with_raydrop(K, _pose(), H, W, lambda images: torch.zeros(1, 1, H, W + 1, device="cuda"))


def test_refusals():
    from lidarnerf.nvs import MeshNVS
    scene, nvs, cloud, inten = _setup()
    with pytest.raises(ValueError, match="intensities for"):
        MeshNVS(scene, cloud, inten[:-1])
    with pytest.raises(ValueError, match="k must be"):
        MeshNVS(scene, cloud, inten, intensity_interpolate_k=17)
    with pytest.raises(ValueError, match=r"\[4, 4\]"):
        nvs.predict_frame(K, np.eye(3), 4, 8)
    bad = cloud.copy()
    bad[5, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        MeshNVS(scene, bad, inten)
    assert MeshNVS(scene, cloud, inten, grid_resolution=(3, 4, 5)).index.grid == (3, 4, 5)


# ----------------------------------------------------------------------------------------------------------- the trainer
RENDER = dict(num_steps=768, upsample_steps=64)
MESH_R = 32


def _trainer(graph=False, rays=1024, **kw):
    """The small model and batches of tests/test_raycast_gpu.py's trainer tests."""
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


def _train(graph, with_nvs):
    from lidarnerf.nvs import MeshNVS
    tr, model, batches, poses = _trainer(graph=graph)
    torch.manual_seed(11)
    losses = []
    for s in range(20):
        losses.append(tr.step(*batches[s % 8]).detach().clone())
        if with_nvs and s + 1 == 10:
            captured = (len(tr.capture_ms), len(tr._graphs)) if graph else None
            ptrs = (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version, tr.global_step)
            scene = tr.mesh_scene(resolution=MESH_R, threshold=_median_threshold(tr))
            rng = np.random.default_rng(8)  # (NumPy's generator: torch's stays where training left it)
            lo, hi = np.array(scene.bounds[0]), np.array(scene.bounds[1])
            cloud = rng.uniform(lo, hi, (2000, 3)).astype(np.float32)
            nvs = MeshNVS(scene, cloud, rng.uniform(0, 1, 2000).astype(np.float32), intensity_interpolate_k=9)
            frame = nvs.predict_frame((2.0, 26.9), poses[0], 8, 32)
            n_hit = int(frame["hit_dict"]["masks"].sum())
            assert n_hit > 0 and frame["points"].shape == (n_hit, 3) and bool(torch.isfinite(frame["pano"]).all())
            assert bool(torch.isfinite(frame["point_intensities"]).all()) and 0 < float(frame["point_intensities"].min())
            assert nvs.raydrop_features((2.0, 26.9), poses[0], 8, 32).shape == (1, 10, 8, 32)
            both = nvs.predict_frame_with_raydrop((2.0, 26.9), poses[0], 8, 32, lambda im: torch.ones_like(im[:, :1]))  # keeps everything
            assert bool(torch.equal(both["pano"], frame["pano"]))
            assert ptrs == (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version, tr.global_step)
    torch.cuda.synchronize()
    if graph:
        assert tr.graph and tr.graph_error is None
        if with_nvs:
            assert captured == (len(tr.capture_ms), len(tr._graphs))  # nothing was captured again after the frame
    state = [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()]
    return state + [p.detach().clone() for p in tr.small] + [torch.stack(losses)]


@pytest.mark.parametrize("graph", [False, True])
def test_training_does_not_notice_a_predicted_frame(graph):
    """Twenty steps from one seed with a mesh scene, a MeshNVS and its three calls after the tenth against twenty without:
    table, fp16 copy, Adam moments, optimizer scalars, every MLP matrix and all losses bit for bit."""
    a = _train(graph, False)
    b = _train(graph, True)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), i
    assert torch.isfinite(a[-1]).all()
