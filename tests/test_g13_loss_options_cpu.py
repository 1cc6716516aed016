"""G13 on the CPU: the torch fallback of the loss options against the reference's own Trainer.train_step
(tests/golden/make_g13_loss_options.py), LidarLossOptions, and the argument contract of lnh_lidar_loss_ex (validated
before any launch, so testable without a GPU)."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from lidarnerf.nerf.train_step import LidarLossOptions, lidar_loss, patch_gradient_loss

G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_loss_options.npz")


def _g13():
    z = np.load(G13)
    return z, json.loads(str(z["cases"]))


def _fallback_loss(z, case, depth, image):
    """LidarTrainer.loss's torch path: lidar_loss (+ patch_gradient_loss on patch epochs) with the case's options."""
    ad, ar, ai, ag = (float(a) for a in z["alphas"])
    scale = float(z["scale"])
    gt = torch.from_numpy(z[f"b{case['batch']}_gt"])[None]
    opts = LidarLossOptions(**case["options"])
    loss, pred_depth, gt_depth = lidar_loss({"depth_lidar": depth[None], "image_lidar": image[None]}, gt, ad, ar, ai,
                                            options=opts, scale=scale)
    px, py = case["patch"]
    if px > 1:
        loss = loss + patch_gradient_loss(pred_depth, gt_depth, gt[..., 0], px, py, scale, ag, options=opts)
    return loss


def test_g13_covers_what_it_promises():
    z, cases = _g13()
    opts = [c["options"] for c in cases]
    for slot in ("depth_loss", "raydrop_loss", "intensity_loss"):
        assert {o[slot] for c, o in zip(cases, opts) if c["patch"] == [1, 1]} == {"l1", "mse", "huber", "bce"}, slot
    for patch in ([2, 8], [4, 4]):
        got = {(o["depth_grad_loss"], o["sobel_grad"]) for c, o in zip(cases, opts) if c["patch"] == patch and o["grad_loss"]}
        assert got >= {(g, s) for g in ("l1", "mse", "huber", "bce", "cos") for s in (False, True)}, patch
    assert any(c["batch"] == 4096 for c in cases)
    gt = z["b512_gt"]
    assert (gt[48:64, 0] == 0).all() and (gt[160:176, 0] == 0).all()       # whole dropped patches
    d = z["b512_depth"]
    assert (d[2] == d[1]) and (d[10] == d[9])                                 # |dx| = 0
    gdx = np.abs(np.diff(gt[:, 2].reshape(-1, 8) / z["scale"], axis=1))
    assert (gdx < 0.01).any() and (gdx > 0.01).any()


@pytest.mark.parametrize("name", [c["name"] for c in _g13()[1]])
def test_torch_fallback_reproduces_g13(name):
    z, cases = _g13()
    case = next(c for c in cases if c["name"] == name)
    N = case["batch"]
    depth = torch.from_numpy(z[f"b{N}_depth"]).clone().requires_grad_(True)
    image = torch.from_numpy(z[f"b{N}_image"]).clone().requires_grad_(True)
    loss = _fallback_loss(z, case, depth, image)
    loss.backward()
    np.testing.assert_allclose(loss.item(), z[f"{name}_loss"], rtol=1e-6)
    for got, key in ((depth.grad, "grad_depth"), (image.grad, "grad_image")):
        want = z[f"{name}_{key}"]
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=1e-7 * np.abs(want).max())


def test_options_from_a_reference_namespace():
    ns = argparse.Namespace(depth_loss="huber", raydrop_loss="bce", intensity_loss="l1", depth_grad_loss="cos",
                            grad_loss=False, sobel_grad=True, grad_norm_smooth=True, spatial_smooth=True, tv_loss=True,
                            alpha_grad_norm=0.5, alpha_spatial=0.2, alpha_tv=3, alpha_d=1e3, enable_lidar=True)
    o = LidarLossOptions.from_opt(ns)
    assert o == LidarLossOptions("huber", "bce", "l1", "cos", False, True, True, True, True, 0.5, 0.2, 3.0)
    assert not o.is_default and isinstance(o.alpha_tv, float)
    # the reference CLI's own defaults (store_true flags off: grad_loss too) and an empty namespace
    cli = argparse.Namespace(depth_loss="l1", raydrop_loss="mse", intensity_loss="mse", depth_grad_loss="l1",
                             grad_loss=False, sobel_grad=False, grad_norm_smooth=False, spatial_smooth=False,
                             tv_loss=False, alpha_grad_norm=1, alpha_spatial=0.1, alpha_tv=1)
    assert LidarLossOptions.from_opt(cli) == LidarLossOptions(grad_loss=False)
    assert LidarLossOptions.from_opt(argparse.Namespace()).is_default
    assert LidarLossOptions().is_default and hash(LidarLossOptions()) == hash(LidarLossOptions())


@pytest.mark.parametrize("field,value", [("depth_loss", "cos"), ("raydrop_loss", "l2"), ("intensity_loss", "Huber"),
                                         ("depth_grad_loss", "sobel")])
def test_unknown_names_raise(field, value):
    with pytest.raises(ValueError, match="not one of l1, mse, huber, bce"):
        LidarLossOptions(**{field: value})


def test_huber_needs_the_scale():
    gt = torch.rand(1, 8, 3)
    out = {"depth_lidar": torch.rand(1, 8), "image_lidar": torch.rand(1, 8, 2)}
    with pytest.raises(ValueError, match="scale"):
        lidar_loss(out, gt, options=LidarLossOptions(depth_loss="huber"))


def test_loss_ex_argument_errors_are_reported_without_a_gpu():
    from lidarnerf import _hip
    L = _hip.lib()
    assert L.lnh_version() >= 102
    N = 512
    ws_bytes = int(L.lnh_lidar_loss_ex_workspace_bytes(N))
    assert ws_bytes >= 4 * ((N + 255) // 256) and ws_bytes % 16 == 0

    def run(n=N, ws=ws_bytes, depth=8, **kw):
        o = _hip.loss_options(LidarLossOptions(), 2, 8, 0.01, 0.002, 1000.0, 1.0, 10.0, 100.0)
        for k, v in kw.items():
            setattr(o, k, v)
        rc = L.lnh_lidar_loss_ex(depth, 8, 8, n, C.byref(o), None, 8, ws, 8, 8, 8, None)
        return rc, L.lnh_last_error().decode()

    cases = [
        (dict(depth_loss=4), "unknown depth criterion 4"),
        (dict(raydrop_loss=-1), "unknown raydrop criterion"),
        (dict(intensity_loss=4), "COS only in the grad slot"),
        (dict(grad_loss=5), "unknown grad criterion 5"),
        (dict(n=500), "multiple of px * py"),
        (dict(py=1), "px > 1 needs py >= 2"),
        (dict(depth=None), "null pointer"),
        (dict(ws=4), "workspace of 4 bytes"),
        (dict(flags=64), "unknown flag bits"),
        (dict(scale=0.0), "scale > 0"),
    ]
    for kw, msg in cases:
        rc, err = run(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    rc, err = run(n=1 << 27, px=1, py=1)
    assert rc == -2 and "2^26" in err


def test_old_library_is_refused_by_name(monkeypatch):
    from lidarnerf import _hip
    monkeypatch.setattr(_hip, "_version_ok", set())
    monkeypatch.setattr(_hip.lib(), "lnh_version", lambda: 101)
    with pytest.raises(RuntimeError, match=r"lnh_version\(\) 101; .*needs 102"):
        _hip.require_version(102, "LidarLossOptions other than the defaults")
