"""The fused frame evaluation on the device (csrc/eval_frame.hip, metrics.FrameEvaluator, LidarTrainer.eval_step / test_step
/ evaluate): against G14 (the reference's own eval_step / test_step and meters, tests/golden/make_g14_eval_step.py), against
the untouched RMSEMeter / MAEMeter / DepthMeter classes on a seeded full-size frame, SSIM against the double-precision
metrics.structural_similarity (a restatement of skimage's defaults, unpinned against a real scikit-image build), run-to-run
and captured-graph bit identity, and the trainer methods on a small model.

Bounds: loss 3e-6 relative (tests/test_g8_train_step_gpu.py's); MAE / RMSE 2e-5 relative and DepthMeter's first four rtol
2e-4, atol 1e-4 (what tests/test_metrics_gpu.py holds the existing meters to against G11); SSIM rtol 2e-4, atol 1e-6
(tests/test_metrics_gpu.py:64)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_eval_step.npz"))
CASES = json.loads(str(G["cases"]))
SCALE, INV = float(G["scale"]), float(G["intensity_inv_scale"])
RENDER = dict(num_steps=768, upsample_steps=64)


def _render_of(key):
    base = key.split("_")[0]
    gt = G["gt_k" if base.startswith("k") else "gt_m"]
    image, depth = G[f"{base}_image"].copy(), G[f"{base}_depth"]
    if key.endswith("_low"):
        image[:, 0] *= np.float32(0.49)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (gt, image, depth))


def _evaluator(case, H, W, **kw):
    from lidarnerf import metrics
    from lidarnerf.nerf.train_step import LidarLossOptions
    a = case["alphas"]
    d, r, i = case["criteria"]
    return metrics.FrameEvaluator(H, W, SCALE, intensity_inv_scale=INV, alphas=(a["alpha_d"], a["alpha_r"], a["alpha_i"]),
                                  loss_options=LidarLossOptions(depth_loss=d, raydrop_loss=r, intensity_loss=i),
                                  nerf_mvl=case["nerf_mvl"], **kw)


def _rel(got, want):
    return abs(got - want) / abs(want)


def _clamped_metres(pred_depth, gt, mvl):
    gr = gt[..., 0]
    if mvl:
        gr = gr * (gr != -1)
    return (pred_depth / SCALE).clamp(1e-3, 80), (gt[..., 2] * gr / SCALE).clamp(1e-3, 80)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_frame_evaluator_against_g14(case):
    from lidarnerf import metrics
    ev = tv = None
    ssims = []
    for rec in case["per_frame"]:
        gt, image, depth = _render_of(rec["render"])
        H, W, _ = gt.shape
        if ev is None:
            ev, tv = _evaluator(case, H, W), _evaluator(case, H, W)
        pi, pd, mask = ev.update(image, depth, gt)
        assert pi.shape == pd.shape == mask.shape == (H, W) and pi.dtype == torch.float32
        assert torch.equal(pi.cpu(), torch.from_numpy(G[rec["pred_intensity"]].reshape(H, W)))
        assert torch.equal(pd.cpu(), torch.from_numpy(G[rec["pred_depth"]].reshape(H, W)))
        valid = (gt[..., 0] != -1) if case["nerf_mvl"] else torch.ones_like(mask, dtype=torch.bool)
        assert torch.equal(mask, ((image.reshape(H, W, 2)[..., 0] > 0.5) & valid).float())
        ti, td, tm = tv.update(image, depth, gt, mode="test")
        assert torch.equal(ti.cpu(), torch.from_numpy(G[rec["test_intensity"]].reshape(H, W)))
        assert torch.equal(td.cpu(), torch.from_numpy(G[rec["test_depth"]].reshape(H, W)))
        assert torch.equal(tm, (image.reshape(H, W, 2)[..., 0] > 0.5).float())
        # SSIM: the double-precision restatement of skimage on the same clamped images, over the crop with nerf_mvl
        P, Gd = _clamped_metres(pd, gt, case["nerf_mvl"])
        if case["nerf_mvl"]:
            r0, c0, h, w = (int(v) for v in G["window_m"])
            P, Gd = P[r0:r0 + h, c0:c0 + w], Gd[r0:r0 + h, c0:c0 + w]
        ssims.append(metrics.structural_similarity(P, Gd, data_range=float(Gd.max() - Gd.min())))
    m = ev.measure()
    hist = m["history"]
    assert m["frames"] == len(case["per_frame"]) == len(hist["loss"])
    for k, rec in enumerate(case["per_frame"]):
        print(case["name"], k, "loss", hist["loss"][k], rec["loss"], "depth", hist["depth_rmse"][k], hist["a1"][k], hist["a2"][k],
              hist["a3"][k], rec["depth_errors"], "ssim", hist["ssim"][k], ssims[k])
        assert _rel(hist["loss"][k], rec["loss"]) <= 3e-6
        got = [hist[n][k] for n in ("depth_rmse", "a1", "a2", "a3")]
        np.testing.assert_allclose(got, rec["depth_errors"], rtol=2e-4, atol=1e-4)
        np.testing.assert_allclose(hist["ssim"][k], ssims[k], rtol=2e-4, atol=1e-6)
        if case["nerf_mvl"]:
            assert [int(hist[n][k]) for n in ("crop_r0", "crop_c0", "crop_h", "crop_w")] == [int(v) for v in G["window_m"]]
            assert int(hist["valid"][k]) == rec["crop"][0] * rec["crop"][1]
    print(case["name"], "mae", m["mae"], case["mae"], "rmse", m["rmse"], case["rmse"], "depth", m["depth"], case["depth"])
    assert _rel(m["loss"], np.mean([r["loss"] for r in case["per_frame"]])) <= 3e-6
    assert _rel(m["mae"], case["mae"]) <= 2e-5 and _rel(m["rmse"], case["rmse"]) <= 2e-5
    np.testing.assert_allclose(m["depth"][:4], case["depth"], rtol=2e-4, atol=1e-4)
    np.testing.assert_allclose(m["depth"][4], np.mean(ssims), rtol=2e-4, atol=1e-6)
    # eval_step applies the mask unless alpha_r = 0 or no pixel predicts > 0.5; test_step whenever alpha_r > 0
    masked = 0 if case["name"] in ("all_low", "alpha_r0") else 1
    assert (hist["masked"] == masked).all() and (hist["bad"] == 0).all()
    assert (tv.measure()["history"]["masked"] == (case["alphas"]["alpha_r"] > 0)).all()


def _seeded_frame(seed, H=66, W=1030):
    g = torch.Generator().manual_seed(seed)
    raydrop = (torch.rand(H, W, generator=g) < 0.75).float()
    gt = torch.stack([raydrop, torch.rand(H, W, generator=g), SCALE * (2 + 76 * torch.rand(H, W, generator=g))], -1)
    image = torch.rand(H * W, 2, generator=g)
    image[:, 0] = torch.where((image[:, 0] - 0.5).abs() < 1e-3, image[:, 0] + 0.01, image[:, 0])
    depth = (gt[..., 2] * (1 + 0.05 * torch.randn(H, W, generator=g))).reshape(-1)
    return gt.cuda(), image.cuda(), depth.cuda()


def test_full_size_frame_against_the_existing_meters():
    from lidarnerf import metrics
    H, W = 66, 1030
    ev = metrics.FrameEvaluator(H, W, SCALE, intensity_inv_scale=INV)
    mae, rmse, dm = metrics.MAEMeter(INV), metrics.RMSEMeter(), metrics.DepthMeter(SCALE)
    for seed in (5, 6):
        gt, image, depth = _seeded_frame(seed)
        pi, pd, mask = ev.update(image, depth, gt)
        want_mask = (image.reshape(H, W, 2)[..., 0] > 0.5).float()
        assert torch.equal(mask, want_mask) and torch.equal(pd, depth.reshape(H, W) * want_mask)
        gi, gd = gt[..., 1] * gt[..., 0], gt[..., 2] * gt[..., 0]
        mae.update(pi[None], gi[None]), rmse.update(pi[None], gi[None]), dm.update(pd[None], gd[None])
    m = ev.measure()
    print("fused", m["mae"], m["rmse"], m["depth"], "meters", mae.measure(), rmse.measure(), dm.measure())
    assert _rel(m["mae"], mae.measure()) <= 2e-5 and _rel(m["rmse"], rmse.measure()) <= 2e-5
    np.testing.assert_allclose(m["depth"][:4], dm.measure()[:4], rtol=2e-4, atol=1e-4)
    np.testing.assert_allclose(m["depth"][4], dm.measure()[4], rtol=2e-4, atol=1e-6)
    assert "Depth_error(rmse, a1, a2, a3, ssim)" in ev.report()


def test_non_rectangular_valid_region_is_refused_at_measure():
    from lidarnerf import metrics
    gt, image, depth = _render_of("m0")
    gt = gt.clone()
    r0, c0, _, _ = (int(v) for v in G["window_m"])
    gt[r0 + 2, c0 + 3, 0] = -1.0
    ev = metrics.FrameEvaluator(gt.shape[0], gt.shape[1], SCALE, nerf_mvl=True)
    ev.update(image, depth, gt)
    with pytest.raises(RuntimeError, match="bounding rectangle"):
        ev.measure()


def test_frames_that_cannot_be_averaged_are_refused_also_beyond_the_history():
    from lidarnerf import metrics
    gt, image, depth = _render_of("m0")
    H, W, _ = gt.shape
    ev = metrics.FrameEvaluator(H, W, SCALE, nerf_mvl=True, max_frames=1)
    ev.update(image, depth, gt)
    assert np.isfinite(ev.measure()["depth"]).all()
    none_valid = gt.clone()
    none_valid[..., 0] = -1.0
    ev.update(image, depth, none_valid)          # (the second frame: not in the one-row history)
    with pytest.raises(RuntimeError, match="1 of 2 frames .* beyond the 1 kept"):
        ev.measure()
    ev.clear()
    small = gt.clone()
    small[..., 0] = -1.0
    small[3:8, 10:40, 0] = 1.0                   # a 5 x 30 window: no SSIM window fits
    ev.update(image, depth, small)
    with pytest.raises(RuntimeError, match="frame 0: ssim = nan"):
        ev.measure()
    ev.clear()
    ev.update(image, depth, gt)
    assert ev.measure()["frames"] == 1


def test_mask_without_a_ground_truth_is_the_test_mode_rule():
    from lidarnerf import metrics
    gt, image, depth = _render_of("k0")
    H, W, _ = gt.shape
    for alpha_r in (1.0, 0.0):
        ev = metrics.FrameEvaluator(H, W, SCALE, alphas=(1000.0, alpha_r, 10.0))
        both = ev.mask(torch.cat([image, image]), torch.cat([depth, depth]))       # two frames' rows at once
        want = ev.update(image, depth, gt, mode="test")
        assert all(g.shape == (2 * H, W) and torch.equal(g[:H], w) and torch.equal(g[H:], w) for g, w in zip(both, want))


def test_mask_has_no_minimum_frame_size():
    from lidarnerf import metrics
    g = torch.Generator().manual_seed(3)
    image, depth = torch.rand(2 * 5, 2, generator=g).cuda(), torch.rand(2 * 5, generator=g).cuda()
    pi, pd, m = metrics.FrameEvaluator(2, 5, SCALE).mask(image, depth)
    want = (image[:, 0] > 0.5).float().reshape(2, 5)
    assert torch.equal(m, want) and torch.equal(pi, image[:, 1].reshape(2, 5) * want) and torch.equal(pd, depth.reshape(2, 5) * want)


def test_two_runs_and_a_captured_graph_give_identical_rows():
    from lidarnerf import metrics
    H, W = 66, 1030
    frames = [_seeded_frame(s) for s in (11, 12)]

    def eager():
        ev = metrics.FrameEvaluator(H, W, SCALE, intensity_inv_scale=INV, max_frames=8)
        outs = [torch.stack(ev.update(image, depth, gt)).clone() for gt, image, depth in frames]
        return ev.state.clone(), outs

    s0, o0 = eager()
    s1, o1 = eager()
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)) and all(torch.equal(a, b) for a, b in zip(o0, o1))
    assert int(s0[0, 18]) == 2 and torch.isfinite(s0[:3]).all()

    ev = metrics.FrameEvaluator(H, W, SCALE, intensity_inv_scale=INV, max_frames=8)
    gt_s, image_s, depth_s = (t.clone() for t in frames[0])
    ev.update(image_s, depth_s, gt_s)  # (buffers exist before the capture)
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ev.update(image_s, depth_s, gt_s)
    ev.clear()
    for k, (gt, image, depth) in enumerate(frames):
        gt_s.copy_(gt), image_s.copy_(image), depth_s.copy_(depth)
        graph.replay()
        assert torch.equal(torch.stack(held), o0[k])
    torch.cuda.synchronize()
    assert torch.equal(ev.state.view(torch.int64), s0.view(torch.int64))


def _trainer(graph=False, **kw):
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph, render_kwargs=RENDER, **kw)
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, 1024, 0, dev, (1, 1), "analytic") for s in range(8)]
    return tr, model, batches


def _frame_data(batch, H=8, W=128, mvl=False):
    rays_o, rays_d, gt = batch
    gt = gt.reshape(1, H, W, 3).clone()
    if mvl:
        window = torch.zeros(H, W, dtype=torch.bool, device=gt.device)
        window[1:H, 8:W - 16] = True
        gt[0, ..., 0] = torch.where(window, gt[0, ..., 0], torch.tensor(-1.0, device=gt.device))
    return {"rays_o_lidar": rays_o.reshape(1, H * W, 3), "rays_d_lidar": rays_d.reshape(1, H * W, 3), "images_lidar": gt,
            "H_lidar": H, "W_lidar": W}


def _bits(model):
    return [p.detach().clone() for p in model.parameters()]


@pytest.mark.parametrize("mvl,criteria", [(False, None), (True, None), (False, ("huber", "bce", "l1"))],
                         ids=["kitti", "nerf_mvl", "huber_bce_l1"])
def test_trainer_eval_step_and_test_step_match_a_torch_restatement(mvl, criteria):
    from lidarnerf.nerf.train_step import LidarLossOptions, _criterion
    import bench
    options = None if criteria is None else LidarLossOptions(depth_loss=criteria[0], raydrop_loss=criteria[1],
                                                            intensity_loss=criteria[2])
    tr, model, batches = _trainer(nerf_mvl=mvl, loss_options=options)
    for b in batches[:3]:
        tr.step(*b)
    data = _frame_data(batches[3], mvl=mvl)
    H, W = data["H_lidar"], data["W_lidar"]
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = model.render(data["rays_o_lidar"], data["rays_d_lidar"], cal_lidar_color=True, staged=True, perturb=False, **RENDER)
    got = tr.eval_step(data)
    tst = tr.test_step(data)
    model.train()
    # utils.py:886-977 restated in torch on the same render
    images = data["images_lidar"]
    gt_raydrop = images[..., 0]
    valid = torch.ones_like(gt_raydrop, dtype=torch.bool)
    if mvl:
        valid = gt_raydrop != -1
        gt_raydrop = gt_raydrop * valid
    gt_intensity, gt_depth = images[..., 1] * gt_raydrop, images[..., 2] * gt_raydrop
    pred = out["image_lidar"].float().reshape(1, H, W, 2)
    pred_raydrop, pred_intensity, pred_depth = pred[..., 0], pred[..., 1], out["depth_lidar"].float().reshape(1, H, W)
    mask = (pred_raydrop > 0.5) & valid
    if mask.any():  # (alpha_r = 1 > 0)
        pred_intensity, pred_depth = pred_intensity * mask, pred_depth * mask
    cd, cr, ci = (_criterion(name, bench.SCALE) for name in (criteria or ("l1", "mse", "mse")))
    loss = (1000.0 * cd(pred_depth, gt_depth).mean() + cr(pred_raydrop, gt_raydrop).mean()
            + 10.0 * ci(pred_intensity, gt_intensity).mean())
    crop = (lambda t: t[:, 1:H, 8:W - 16]) if mvl else (lambda t: t)
    want = (crop(pred_intensity).unsqueeze(-1), pred_depth, crop(pred_depth) if mvl else None, pred_raydrop.unsqueeze(-1),
            crop(gt_intensity).unsqueeze(-1), gt_depth, crop(gt_depth) if mvl else None, gt_raydrop.unsqueeze(-1))
    assert len(got) == 9
    for k, (g, w) in enumerate(zip(got[:8], want)):
        if w is None:
            assert g is None, k
        else:
            assert g.shape == w.shape and g.dtype == torch.float32 and torch.equal(g, w), k
    assert got[8].dim() == 0 and got[8].is_cuda and _rel(float(got[8]), float(loss)) <= 3e-6
    t_mask = pred_raydrop > 0.5
    want_t = (pred_raydrop, pred[..., 1] * t_mask, out["depth_lidar"].float().reshape(1, H, W) * t_mask)
    assert len(tst) == 3 and all(g.shape == (1, H, W) and torch.equal(g, w) for g, w in zip(tst, want_t))


def test_evaluate_runs_on_the_averaged_weights_and_leaves_training_untouched():
    def run(graph, evaluate_at, ema_arg=True, boom=False):
        tr, model, batches = _trainer(graph=graph, ema_decay=0.95, ema_interval=1)
        frames = [_frame_data(b) for b in batches[5:7]]
        results = []
        for k, b in enumerate(batches[:5]):
            tr.step(*b)
            if k == evaluate_at:
                before = _bits(model)
                if boom:
                    with pytest.raises(KeyError):
                        tr.evaluate(frames + [{"rays_o_lidar": frames[0]["rays_o_lidar"]}])
                else:
                    results.append(tr.evaluate(frames, ema=ema_arg))
                assert model.training and all(torch.equal(a, b) for a, b in zip(before, _bits(model)))
        torch.cuda.synchronize()
        return tr, _bits(model), results

    for graph in (False, True):
        _, plain, _ = run(graph, None)
        tr, with_eval, res = run(graph, 2)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, with_eval)), graph
        r = res[0]
        assert r["frames"] == 2 and np.isfinite(r["loss"]) and np.isfinite(r["depth"]).all()
        assert tr.stats["valid_loss"] == [r["loss"]] and tr.stats["results"] == [float(r["depth"][0])]
    _, after_boom, _ = run(False, 2, boom=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, after_boom))
    _, _, on_ema = run(False, 4)
    _, _, on_raw = run(False, 4, ema_arg=False)
    assert on_ema[0]["loss"] != on_raw[0]["loss"]


def test_evaluate_with_the_points_meter_reports_the_chamfer_distance(tmp_path):
    import bench
    tr, model, batches = _trainer()
    for b in batches[:3]:
        tr.step(*b)
    frames = [_frame_data(b) for b in batches[3:5]]
    r = tr.evaluate(frames, points_intrinsics=bench.INTRINSICS, save_dir=str(tmp_path))
    assert tr.stats["results"] == [float(r["points"][0])] and np.isfinite(r["points"]).all()
    assert sorted(os.listdir(tmp_path)) == ["ep0000_0001_lidar.npy", "ep0000_0002_lidar.npy"]
    assert np.load(os.path.join(tmp_path, "ep0000_0001_lidar.npy")).shape[1] == 3
