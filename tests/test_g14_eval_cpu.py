"""G14 on the CPU: the NumPy restatement of the frame evaluation (tests/eval_frame_ref.py) against what the reference's OWN
Trainer.eval_step / test_step and MAEMeter / RMSEMeter / DepthMeter computed on the same renders
(tests/golden/make_g14_eval_step.py; SSIM is not in the fixture: scikit-image was not installed where the reference ran);
the argument checks of the lnh_lidar_eval_* entry points, which happen before any launch; and the Python surface —
metrics.FrameEvaluator, LidarTrainer.eval_step / test_step / evaluate — with its refusal of CPU tensors."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import eval_frame_ref as ref

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_eval_step.npz"))
CASES = json.loads(str(G["cases"]))
INVALID_ARG, UNSUPPORTED = -1, -2  # LNH_ERR_INVALID_ARG, LNH_ERR_UNSUPPORTED (include/lidarnerf_hip.h)
SCALE, INV = float(G["scale"]), float(G["intensity_inv_scale"])


def render_of(key):
    base = key.split("_")[0]
    gt = G["gt_k" if base.startswith("k") else "gt_m"]
    image, depth = G[f"{base}_image"].copy(), G[f"{base}_depth"]
    if key.endswith("_low"):
        image[:, 0] *= np.float32(0.49)
    return gt, image, depth


def close(got, want, rel):
    return abs(got - want) <= rel * abs(want)


def test_fixture_holds_the_cases_the_rules_need():
    names = {c["name"] for c in CASES}
    assert {"default", "all_low", "alpha_r0", "nerf_mvl", "huber_bce_l1", "clamps", "two_frames"} <= names
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_eval_step.npz")) <= 1 << 20
    for key in ("k0", "k1", "m0"):
        assert np.abs(G[f"{key}_image"][:, 0] - 0.5).min() >= 1e-3
    assert (render_of("k0_low")[1][:, 0] <= 0.5 - 1e-3).all()
    metres = G["k1_depth"][:4] / np.float32(SCALE)
    np.testing.assert_allclose(metres, [0.0, 1e-4, 80.0, 100.0], rtol=1e-6)
    assert (G["gt_m"][..., 0] == -1).any() and not (G["gt_k"][..., 0] == -1).any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    a = case["alphas"]
    alphas = (a["alpha_d"], a["alpha_r"], a["alpha_i"])
    maes, rmses, depths = [], [], []
    for rec in case["per_frame"]:
        gt, image, depth = render_of(rec["render"])
        H, W, _ = gt.shape
        step = ref.eval_step(image, depth, gt, alphas=alphas, scale=SCALE, criteria=case["criteria"], nerf_mvl=case["nerf_mvl"])
        # masked images: products with 0 / 1, bit-exact
        assert np.array_equal(step["pred_intensity"], G[rec["pred_intensity"]].reshape(H, W))
        assert np.array_equal(step["pred_depth"], G[rec["pred_depth"]].reshape(H, W))
        t = ref.test_step(image, depth, H, W, alpha_r=a["alpha_r"])
        assert np.array_equal(t[1], G[rec["test_intensity"]].reshape(H, W))
        assert np.array_equal(t[2], G[rec["test_depth"]].reshape(H, W))
        assert close(step["loss"], rec["loss"], 1e-6), (step["loss"], rec["loss"])
        if case["nerf_mvl"]:
            assert list(step["pred_depth_crop"].shape) == rec["crop"] == list(G["window_m"][2:])
        else:
            assert rec["crop"] is None and step["pred_depth_crop"] is None
        mae, rmse, d = ref.frame_meters(step, scale=SCALE, intensity_inv_scale=INV)
        np.testing.assert_allclose(d, rec["depth_errors"], rtol=1e-6, atol=0)
        maes.append(mae), rmses.append(rmse), depths.append(d)
    assert close(np.mean(maes), case["mae"], 1e-6) and close(np.mean(rmses), case["rmse"], 1e-6)
    np.testing.assert_allclose(np.mean(depths, axis=0), case["depth"], rtol=1e-6, atol=0)


def test_masking_branches_are_exercised():
    by = {c["name"]: c for c in CASES}
    low, default, r0 = by["all_low"]["per_frame"][0], by["default"]["per_frame"][0], by["alpha_r0"]["per_frame"][0]
    assert low["pred_depth"] == "k0_depth" and r0["pred_depth"] == "k0_depth"       # eval_step left them unmasked
    assert default["pred_depth"] != "k0_depth" and default["test_depth"] == default["pred_depth"]
    assert not G[low["test_intensity"]].any() and low["test_depth"] == low["test_intensity"]  # test_step masked everything
    assert r0["test_depth"] == "k0_depth"
    two = by["two_frames"]
    assert close(two["rmse"], (by["default"]["rmse"] + by["clamps"]["rmse"]) / 2, 1e-6)  # mean of per-frame values


def _options(**kw):
    from lidarnerf import _hip
    from lidarnerf.nerf.train_step import LidarLossOptions
    o = LidarLossOptions(**{k: v for k, v in kw.items() if k.endswith("_loss")})
    return _hip.loss_options(o, 1, 1, kw.get("scale", SCALE), 0.2 * SCALE, 1000.0, 1.0, 10.0, 0.0)


def test_entry_points_check_arguments_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    H, W = 24, 515
    need = L.lnh_lidar_eval_workspace_bytes(H, W)
    assert need > 0
    for h, w in ((6, 515), (24, 6), (0, 0)):
        assert L.lnh_lidar_eval_workspace_bytes(h, w) == 0
    buf = (C.c_double * (need // 8 + 1))()
    ws = C.addressof(buf)
    opt = _options()
    po = C.addressof(opt)
    x = 8  # any non-null, aligned value: every call below must fail before it is dereferenced

    def frame(image=x, depth=x, gt=x, h=H, w=W, o=po, mode=0, wsp=ws, wsb=need, oi=x, od=x, om=x):
        return L.lnh_lidar_eval_frame(image, depth, gt, h, w, o, 1.0, mode, 0, wsp, wsb, oi, od, om, None)

    for kw, word in ((dict(image=None), "image_lidar"), (dict(depth=None), "depth_lidar"), (dict(gt=None), "gt"),
                     (dict(oi=None), "pred_intensity"), (dict(o=None), "options"), (dict(h=6), "H"), (dict(w=5), "W"),
                     (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(wsp=None), "workspace"),
                     (dict(wsb=need - 8), "workspace")):
        assert frame(**kw) == INVALID_ARG and word in err(), (kw, err())
    for slot in ("depth_loss", "raydrop_loss", "intensity_loss"):
        bad = _options()
        setattr(bad, slot, _hip.LOSS_CODES["cos"])
        assert frame(o=C.addressof(bad)) == INVALID_ARG and "cos" in err() and slot.split("_")[0] in err(), err()
        setattr(bad, slot, 7)
        assert frame(o=C.addressof(bad)) == INVALID_ARG and "criterion" in err()
    # gt == NULL: the mask-only path of test_step (LNH_EVAL_MODE_TEST only), any H, W >= 1, no workspace
    for kw, code, word in ((dict(gt=None, mode=0), INVALID_ARG, "gt"), (dict(gt=None, mode=1, h=0, wsp=None, wsb=0), INVALID_ARG, "H"),
                           (dict(gt=None, mode=1, w=0, wsp=None, wsb=0), INVALID_ARG, "W"),
                           (dict(gt=None, mode=1, h=1 << 13, w=1 << 12, wsp=None, wsb=0), UNSUPPORTED, "2^24"),
                           (dict(gt=None, mode=1, oi=None, wsp=None, wsb=0), INVALID_ARG, "pred_intensity"),
                           (dict(gt=None, mode=1, o=None, wsp=None, wsb=0), INVALID_ARG, "options")):
        assert frame(**kw) == code and word in err(), (kw, err())
    assert frame(h=1 << 13, w=1 << 12) == UNSUPPORTED and "2^24" in err()   # (the same code with a ground truth)
    zero_scale = _options(scale=0.0)
    assert frame(o=C.addressof(zero_scale)) == INVALID_ARG and "scale" in err()

    def ssim(pred=x, gt=x, h=H, w=W, scale=SCALE, wsp=ws, wsb=need):
        return L.lnh_lidar_eval_ssim(pred, gt, h, w, scale, 0, wsp, wsb, None)

    for kw, word in ((dict(pred=None), "pred_depth"), (dict(gt=None), "gt"), (dict(h=3), "H"), (dict(w=6), "W"),
                     (dict(scale=0.0), "scale"), (dict(wsb=0), "workspace")):
        assert ssim(**kw) == INVALID_ARG and word in err(), (kw, err())

    def finalize(h=H, w=W, o=po, mode=0, wsp=ws, wsb=need, acc=x, hist=x, frames=4):
        return L.lnh_lidar_eval_finalize(h, w, o, mode, 0, wsp, wsb, acc, hist, frames, None)

    for kw, word in ((dict(acc=None), "accumulator"), (dict(hist=None), "history"), (dict(o=None), "options"), (dict(h=6), "H"),
                     (dict(mode=5), "mode"), (dict(wsp=None), "workspace"), (dict(acc=12), "aligned")):
        assert finalize(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert L.lnh_version() == 102 and len(_hip.EVAL_SLOT_NAMES) == _hip.EVAL_SLOTS == 20


def test_header_slot_layout_matches_the_binding():
    import re
    from lidarnerf import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lidarnerf_hip.h")).read()
    slots = dict((n.lower(), int(v)) for n, v in re.findall(r"LNH_EVAL_(?!MODE)(\w+) = (\d+)", text))
    assert slots.pop("slots") == _hip.EVAL_SLOTS
    assert [k for k, _ in sorted(slots.items(), key=lambda kv: kv[1])] == list(_hip.EVAL_SLOT_NAMES)
    modes = dict((n.lower(), int(v)) for n, v in re.findall(r"LNH_EVAL_MODE_(\w+) = (\d+)", text))
    assert modes == _hip.EVAL_MODES


def test_python_surface_and_no_cpu_fallback():
    from lidarnerf import metrics
    from lidarnerf.nerf.train_step import LidarLossOptions, LidarTrainer
    sig = inspect.signature(metrics.FrameEvaluator.__init__)
    assert list(sig.parameters)[1:] == ["H", "W", "scale", "intensity_inv_scale", "alphas", "loss_options", "nerf_mvl",
                                        "max_frames"]
    assert sig.parameters["intensity_inv_scale"].default == 1.0 and sig.parameters["nerf_mvl"].default is False
    assert list(inspect.signature(metrics.FrameEvaluator.update).parameters)[1:] == ["image_lidar", "depth_lidar",
                                                                                     "images_lidar", "mode"]
    assert inspect.signature(metrics.FrameEvaluator.update).parameters["mode"].default == "eval"
    for name in ("measure", "clear", "report"):
        assert callable(getattr(metrics.FrameEvaluator, name))
    assert list(inspect.signature(LidarTrainer.eval_step).parameters) == ["self", "data"]
    p = inspect.signature(LidarTrainer.test_step).parameters
    assert list(p) == ["self", "data", "perturb"] and p["perturb"].default is False
    p = inspect.signature(LidarTrainer.evaluate).parameters
    assert list(p) == ["self", "frames", "points_intrinsics", "ema", "save_dir"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("points_intrinsics", "ema", "save_dir"))
    assert p["ema"].default is True and p["points_intrinsics"].default is None and p["save_dir"].default is None

    H, W = 24, 515
    ev = metrics.FrameEvaluator(H, W, SCALE, loss_options=LidarLossOptions(depth_loss="huber"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(torch.zeros(H * W, 2), torch.zeros(H * W), torch.zeros(H, W, 3))
    with pytest.raises(ValueError, match="mode"):
        ev.update(torch.zeros(H * W, 2), torch.zeros(H * W), torch.zeros(H, W, 3), mode="train")
    with pytest.raises(RuntimeError, match="no frame"):
        ev.measure()
    with pytest.raises(ValueError, match="at least 7"):  # (update() needs the SSIM window; mask() / test_step do not)
        metrics.FrameEvaluator(6, 515, SCALE).update(torch.zeros(6 * 515, 2), torch.zeros(6 * 515), torch.zeros(6, 515, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.FrameEvaluator(2, 5, SCALE).mask(torch.zeros(10, 2), torch.zeros(10))
    with pytest.raises(ValueError, match="positive"):
        metrics.FrameEvaluator(0, 515, SCALE)
    with pytest.raises(TypeError):
        metrics.FrameEvaluator(H, W, SCALE, loss_options="huber")

    class _Field(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(3))

        def get_params(self, lr):
            return [{"params": [self.w], "lr": lr}]

    tr = LidarTrainer(_Field(), fp16=False, scale=SCALE)
    assert tr.nerf_mvl is False and tr.intensity_inv_scale == 1.0
    data = {"rays_o_lidar": torch.zeros(1, H * W, 3), "rays_d_lidar": torch.zeros(1, H * W, 3),
            "images_lidar": torch.zeros(1, H, W, 3), "H_lidar": H, "W_lidar": W}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.eval_step(data)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.test_step(data)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.evaluate([data])
    assert tr.model.training and tr.stats["valid_loss"] == [] and tr.stats["results"] == []
