"""Device-side batch sampler on the GPU (csrc/lidar_sample.hip, dataset/sampler.py, LidarTrainer.step_sampled /
train_epoch): indices bit for bit against the NumPy restatement (tests/sampler_ref.py), origins and targets bit for bit,
directions against float64 within twice get_lidar_rays' own deviation, the full-frame rays against the G3 golden, bounds,
patch layout and uniformity over 256 draws, the cursor (eager = graph replay), streams, state round trip, and training
through step_sampled = training through step() on the same draws, bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import sampler_ref as ref

pytestmark = pytest.mark.gpu
INTR = (2.0, 26.9)
SCALE = 0.010784853507573345
ULP4 = 4 * 2.0 ** -23  # 4 ulp of 1.0: the floor of the direction bound


def _sequence(F=3, H=8, W=12, dtype=torch.float16, seed=0, scale=SCALE):
    """F frames with random rotations (QR of a Gaussian matrix), translations inside the unit cube's middle, targets shaped
    like load_sequence's (ray-drop, intensity, depth * scale)."""
    g = torch.Generator().manual_seed(seed)
    poses = torch.eye(4).repeat(F, 1, 1)
    for k in range(F):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        poses[k, :3, :3] = q
        poses[k, :3, 3] = (torch.rand(3, generator=g) - 0.5) * 0.2
    drop = (torch.rand(F, H, W, generator=g) < 0.8).float()
    images = torch.stack([drop, torch.rand(F, H, W, generator=g), scale * (2 + 30 * torch.rand(F, H, W, generator=g))], -1)
    return {"poses_lidar": poses.cuda(), "images_lidar": images.to(dtype).cuda(), "H_lidar": H, "W_lidar": W}


def _sampler(seq=None, **kw):
    from lidarnerf.dataset.sampler import LidarBatchSampler
    return LidarBatchSampler(seq if seq is not None else _sequence(), INTR, **kw)


def _take(s, k):
    """k draws, each cloned: [(rays_o, rays_d, gt, inds)]."""
    out = []
    for _ in range(k):
        o, d, gt = s.draw()
        out.append((o[0].clone(), d[0].clone(), gt[0].clone(), s.inds.clone()))
    return out


CASES = {"1x1": (8, 12, 1, 16, 16), "2x4": (8, 12, [2, 4], 70, 64), "flat": (8, 12, 0, 16, 16), "clamped": (8, 12, 1, 200, 96),
         "bench2x8": (66, 1030, [2, 8], 4096, 4096)}
SEED, STREAM = 0x1234567811, 2


@functools.lru_cache(maxsize=None)
def _drawn(case, dtype):
    """Three draws of one case in file order (no new_epoch: draw k reads frame k), computed once and left unchanged."""
    H, W, ps, N, n = CASES[case]
    seq = _sequence(3, H, W, dtype)
    s = _sampler(seq, num_rays=N, patch_size=ps, seed=SEED, stream_id=STREAM)
    assert s.n == n
    draws = _take(s, 3)
    torch.cuda.synchronize()
    return seq, s, draws


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", list(CASES))
def test_indices_match_the_restatement(case, dtype):
    H, W, ps, N, n = CASES[case]
    _, s, draws = _drawn(case, dtype)
    for k, (_, _, _, inds) in enumerate(draws):
        want = ref.batch_indices(N, H, W, s.px, s.py, SEED, k, STREAM)
        assert inds.dtype == torch.int32 and inds.shape == (n,)
        np.testing.assert_array_equal(inds.cpu().numpy().astype(np.int64), want)
    assert s.cursor.tolist() == [3, 3]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", list(CASES))
def test_origins_and_targets_are_bit_exact(case, dtype):
    seq, s, draws = _drawn(case, dtype)
    for k, (o, _, gt, inds) in enumerate(draws):
        assert o.dtype == torch.float32 and gt.dtype == dtype
        assert torch.equal(o, seq["poses_lidar"][k, :3, 3].expand_as(o))
        flat = seq["images_lidar"][k].reshape(-1, 3)
        assert torch.equal(gt, torch.gather(flat, 0, inds.long()[:, None].expand(-1, 3)))


@pytest.mark.parametrize("case", list(CASES))
def test_directions_are_as_accurate_as_get_lidar_rays(case):
    """|rays_d - float64| <= max(2 x the largest deviation of get_lidar_rays from the same float64 restatement on the same
    pixels, 4 ulp of 1.0): the kernel may not be less accurate than the torch path it replaces, up to summation order."""
    from lidarnerf.dataset.rays import get_lidar_rays
    H, W = CASES[case][:2]
    seq, s, draws = _drawn(case, torch.float16)
    for k, (_, d, _, inds) in enumerate(draws):
        pose = seq["poses_lidar"][k]
        want = ref.directions(inds.cpu().numpy(), pose.cpu().numpy(), H, W, *INTR)
        torch_d = get_lidar_rays(pose[None], INTR, H, W, -1)["rays_d"][0][inds.long()]
        dev_torch = np.abs(torch_d.cpu().numpy().astype(np.float64) - want).max()
        dev_kernel = np.abs(d.cpu().numpy().astype(np.float64) - want).max()
        print(f"[sampler directions] {case} draw {k}: kernel {dev_kernel:.3e}  get_lidar_rays {dev_torch:.3e}")
        assert dev_kernel <= max(2 * dev_torch, ULP4), (dev_kernel, dev_torch)


def test_full_frame_rays_match_the_g3_golden(golden_dir):
    """lnh_lidar_frame_rays against the reference's get_lidar_rays outputs (tests/golden/g3_lidar_rays.npz), at the
    tolerance tests/test_rays_cpu.py holds the torch restatement to."""
    g = np.load(os.path.join(golden_dir, "g3_lidar_rays.npz"))
    pose = torch.from_numpy(g["pose"]).reshape(-1, 4, 4).float()
    for (H, W, intr, sel, want_d, want_o) in ((66, 1030, (2.0, 26.9), g["sel"], g["rays_d"], g["rays_o"]),
                                              (256, 1800, (15.0, 40.0), g["mvl_sel"], g["mvl_rays_d"], None)):
        from lidarnerf.dataset.sampler import LidarBatchSampler
        seq = {"poses_lidar": pose.cuda(), "images_lidar": torch.zeros(pose.shape[0], H, W, 3, device="cuda"), "H_lidar": H,
               "W_lidar": W}
        data = LidarBatchSampler(seq, intr, num_rays=16).frame(0)
        assert data["rays_d_lidar"].shape == (1, H * W, 3) and data["images_lidar"].shape == (1, H, W, 3)
        assert (data["H_lidar"], data["W_lidar"]) == (H, W)
        np.testing.assert_allclose(data["rays_d_lidar"][0].cpu().numpy()[sel], want_d, rtol=0, atol=1e-6)
        if want_o is not None:
            np.testing.assert_array_equal(data["rays_o_lidar"][0].cpu().numpy()[sel], want_o)
    frames = list(LidarBatchSampler(_sequence(), INTR, num_rays=16).frames())
    assert len(frames) == 3 and not torch.equal(frames[0]["rays_d_lidar"], frames[1]["rays_d_lidar"])


@pytest.mark.parametrize("ps,N", [(1, 96), ([2, 4], 96), ([7, 11], 96), ([3, 1], 50)])
def test_bounds_and_patch_layout_over_256_draws(ps, N):
    H, W = 8, 12
    s = _sampler(num_rays=N, patch_size=ps, seed=3)
    px, py = s.px, s.py
    inds = torch.stack([s.draw() and s.inds.clone() for _ in range(256)]).long().reshape(-1, px * py)
    corner = inds[:, 0]
    assert int((corner // W).max()) < H - px and int((corner % W).max()) < W - py and int(corner.min()) >= 0
    k = torch.arange(px * py, device="cuda")
    assert torch.equal(inds - corner[:, None], ((k // py) * W + k % py).expand_as(inds))
    assert int(inds.max()) < H * W
    if (px, py) != (7, 11):  # (a single possible corner otherwise)
        assert len(torch.unique(corner)) > 1


def test_uniformity_of_corners():
    """1 x 1, seed 0, 256 draws asking for 4096 rays of an 8 x 12 image (clamped to 96 each): every one of the 77 corner
    cells within 5 sigma of its binomial expectation.  Deterministic; tests/test_sampler_cpu.py holds the restatement to the
    same bound for this seed."""
    from test_sampler_cpu import check_uniform
    H, W = 8, 12
    s = _sampler(num_rays=4096, patch_size=1, seed=0)
    inds = torch.stack([s.draw() and s.inds.clone() for _ in range(256)]).long().reshape(-1)
    cell = (inds // W) * (W - 1) + inds % W
    assert int((inds // W).max()) < H - 1 and int((inds % W).max()) < W - 1
    check_uniform(torch.bincount(cell, minlength=77).cpu().numpy(), 256 * 96)


def test_cursor_frames_follow_perm_and_epochs():
    seq = _sequence(F=3)
    s = _sampler(seq, num_rays=16, seed=7)
    t = seq["poses_lidar"][:, :3, 3]
    seen = []
    for epoch in (1, 2):
        s.new_epoch()
        perm = s.perm.tolist()
        assert sorted(perm) == [0, 1, 2] and s.epoch == epoch
        assert s.cursor.tolist()[0] == 0
        for step in range(5):  # (past the end of the epoch: the order wraps)
            o, _, _ = s.draw()
            assert torch.equal(o[0, 0], t[perm[step % 3]])
            seen.append(s.cursor.tolist())
    assert [c[0] for c in seen] == [1, 2, 3, 4, 5] * 2 and [c[1] for c in seen] == list(range(1, 11))  # never repeats
    # an explicit frame: that frame, the counters advance all the same
    o, _, _ = s.draw(frame=2)
    assert torch.equal(o[0, 0], t[2]) and s.cursor.tolist() == [6, 11]
    # another seed, another order somewhere in the first epochs
    other = _sampler(seq, num_rays=16, seed=8)
    orders = [[smp._permutation(e).tolist() for e in range(1, 9)] for smp in (s, other)]
    assert orders[0] != orders[1]


def test_eager_draws_equal_graph_replays():
    """K = 5 eager draws = K replays of a torch.cuda.graph holding ONE draw, bit for bit: frame and random stream are read
    from device memory, nothing of them is frozen into the captured launch.  The cursor reads K after either."""
    K = 5
    seq = _sequence(F=3)
    a, b = (_sampler(seq, num_rays=70, patch_size=[2, 4], seed=21) for _ in range(2))
    _sampler(seq, num_rays=70, patch_size=[2, 4]).draw()  # (the kernels' code is loaded before anything is captured)
    for s in (a, b):
        s.new_epoch()
    eager = _take(a, K)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.draw()
    assert b.cursor.tolist() == [0, 0]  # (captured, not run)
    for k in range(K):
        graph.replay()
        got = (b.rays_o, b.rays_d, b.gt, b.inds)
        for x, y in zip(eager[k], got):
            assert torch.equal(x, y), k
    assert a.cursor.tolist() == [K, K] == b.cursor.tolist()
    assert not torch.equal(eager[0][3], eager[1][3])


def test_streams_and_seeds():
    seq = _sequence()
    base = _take(_sampler(seq, num_rays=64, seed=5, stream_id=0), 3)
    same = _take(_sampler(seq, num_rays=64, seed=5, stream_id=0), 3)
    rank1 = _take(_sampler(seq, num_rays=64, seed=5, stream_id=1), 3)
    seed6 = _take(_sampler(seq, num_rays=64, seed=6, stream_id=0), 3)
    for k in range(3):
        assert all(torch.equal(x, y) for x, y in zip(base[k], same[k]))
        assert not torch.equal(base[k][3], rank1[k][3]) and not torch.equal(base[k][3], seed6[k][3])
        np.testing.assert_array_equal(rank1[k][3].cpu().numpy(), ref.batch_indices(64, 8, 12, 1, 1, 5, k, 1))


def test_state_round_trip_mid_epoch():
    seq = _sequence(F=3)
    a = _sampler(seq, num_rays=70, patch_size=[2, 4], seed=33, stream_id=1)
    a.new_epoch()
    a.new_epoch()
    _take(a, 2)
    sd = a.state_dict()
    assert (sd["seed"], sd["stream_id"], sd["epoch"], sd["step"], sd["draws"]) == (33, 1, 2, 2, 2) and len(sd["perm"]) == 3
    b = _sampler(seq, num_rays=70, patch_size=[2, 4], seed=1)
    b.load_state_dict(sd)
    for smp in (a, b):
        smp.rest = _take(smp, 4)  # (to the end of the epoch and past it)
        smp.new_epoch()
        smp.rest += _take(smp, 3)
    assert a.perm.tolist() == b.perm.tolist() and a.cursor.tolist() == b.cursor.tolist() == [3, 9]
    for x, y in zip(a.rest, b.rest):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    # set_patch: other buffers, the same cursor and order
    before, perm = a.cursor.tolist(), a.perm.tolist()
    a.set_patch(16, 1)
    assert a.n == 16 and a.rays_o.shape == (16, 3) and a.cursor.tolist() == before and a.perm.tolist() == perm
    a.draw()
    np.testing.assert_array_equal(a.inds.cpu().numpy(), ref.batch_indices(16, 8, 12, 1, 1, 33, 9, 1))


# ---------------------------------------------------------------------------------------------------- the trainer
def _trainer(occupancy, graph):
    from lidarnerf.nerf.train_step import LidarTrainer
    torch.manual_seed(0)
    if occupancy:
        from lidarnerf.nerf.network import NeRFNetwork
        net = NeRFNetwork(encoding="hashgrid", desired_resolution=2048, bound=1, min_near=SCALE, min_near_lidar=SCALE,
                          density_thresh=10, cuda_ray=True)
        with torch.no_grad():
            net.encoder.embeddings.uniform_(-0.5, 0.5)
        net = net.cuda().train()
        tr = LidarTrainer(net, lr=1e-2, iters=30000, fp16=True, scale=SCALE, graph=graph, render_kwargs={})
    else:
        import bench
        net = bench.build_model(torch.device("cuda", 0))
        tr = LidarTrainer(net, lr=1e-2, iters=30000, fp16=True, scale=SCALE, graph=graph,
                          render_kwargs=dict(num_steps=768, upsample_steps=64))
    assert tr.table is not None and tr.graph == graph and tr.occupancy == occupancy
    return tr


def _state(tr, losses):
    torch.cuda.synchronize()
    return [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()] + \
        [p.detach().clone() for p in tr.small] + [torch.stack(losses)]


# Rays per training batch.  Dense path: 64.  Occupancy path: 16, the rays of ONE workgroup of the training marcher
# (csrc/raymarch.hip, kMarchRaysPerGroup): its workgroups reserve their sample rows with a device atomic, in arrival order,
# and the weight gradients are added up along the sample rows — with more than one workgroup two runs of the SAME step()
# calls already differ in the last bits (tests/test_lidar_infer_gpu.py says so of its training gradient), and "step_sampled
# = step on the same draws, bit for bit" would be a statement about that order, not about the sampler.  One workgroup has
# one order.  (The draw kernel over several workgroups: the index tests above.)
TRAIN_RAYS = {False: 64, True: 16}


def _run(occupancy, graph, ps, steps, sampled):
    seq = _sequence(F=3, seed=4)
    s = _sampler(seq, num_rays=TRAIN_RAYS[occupancy], patch_size=ps, seed=17)
    s.new_epoch()
    tr = _trainer(occupancy, graph)
    torch.manual_seed(11)
    losses = []
    for _ in range(steps):
        loss = tr.step_sampled(s) if sampled else tr.step(*s.draw(), s.patch)
        losses.append(loss.detach().clone())
    assert s.cursor.tolist() == [steps, steps] and tr.global_step == steps  # no step drawn twice or skipped
    return tr, _state(tr, losses)


@pytest.mark.parametrize("ps", [1, [2, 4]])
@pytest.mark.parametrize("occupancy", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_step_sampled_equals_step_on_the_same_draws(graph, occupancy, ps):
    """6 steps of step_sampled(s1) against 6 steps of step(*s2.draw(), patch), s2 a sampler of the same seed: losses, table,
    fp16 copy, Adam moments, optimizer scalars and every MLP matrix bit for bit."""
    tr, a = _run(occupancy, graph, ps, 6, sampled=True)
    _, b = _run(occupancy, graph, ps, 6, sampled=False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
    assert torch.isfinite(a[-1]).all() and float(a[4][0]) > 0
    if graph:
        assert tr.graph and tr.graph_error is None
        if not occupancy:  # (the occupancy step is captured once the marcher has a sample mean: the test below)
            assert len(tr._graphs) == 1 and len(tr.capture_ms) == 1


def test_step_sampled_through_the_occupancy_capacity_ladder():
    """40 steps on the occupancy path with graph=True: 16 launch by launch (no sample mean yet), then captured steps that
    share the sampler's cursor — the same bits as step() on the same draws, and exactly 40 draws."""
    tr, a = _run(True, True, 1, 40, sampled=True)
    _, b = _run(True, True, 1, 40, sampled=False)
    assert tr.graph and tr.graph_error is None and len(tr._graphs) >= 1
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


@pytest.mark.parametrize("graph", [False, True])
def test_train_epoch(graph):
    _, a = _run(False, graph, 1, 6, sampled=True)
    s = _sampler(_sequence(F=3, seed=4), num_rays=64, patch_size=1, seed=17)
    tr = _trainer(False, graph)
    torch.manual_seed(11)
    mean = tr.train_epoch(s, steps=6)
    total = a[-1][0].float().cpu()
    for x in a[-1][1:].float().cpu():
        total = total + x
    assert mean == float(total) / 6  # (the fp32 sum in step order, divided on the host)
    assert tr.epoch == 1 and tr.stats["loss"] == [mean] and tr.global_step == 6 and s.cursor.tolist() == [6, 6]
    assert tr.train_epoch(s) < float("inf") and tr.epoch == 2 and tr.global_step == 9 and s.epoch == 2  # F = 3 steps
    b = _state(tr, [torch.zeros((), device="cuda")])
    assert not torch.equal(a[0], b[0])
