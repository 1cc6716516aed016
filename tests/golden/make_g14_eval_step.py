#!/usr/bin/env python3
"""G14: the reference's Trainer.eval_step / test_step and its evaluation meters on fixed renders (CPU).

    python tests/golden/make_g14_eval_step.py <reference checkout>

The G8 / G13 recipe (make_golden._reference_trainer()): the reference's OWN Trainer.eval_step and Trainer.test_step
(lidarnerf/nerf/utils.py:886-1009), called unbound on a stub `self` whose model.render returns fixed tensors, and its OWN
MAEMeter, RMSEMeter and DepthMeter (226-362) fed with what eval_step returned, in the order and with the crop rule of
evaluate_one_epoch (1357-1366).  scikit-image is not installed where this runs: `structural_similarity` is a placeholder
that returns NaN, so SSIM is NOT in the fixture (as in G11) — of DepthMeter's five numbers the first four are pinned.

Writes g14_eval_step.npz next to this script: numeric arrays and one JSON case list.  Two input frames are shared by the
cases: `k` (24 x 515, KITTI-360-style: every pixel inside the sensor's window) with two renders k0 / k1 of it, and `m`
(32 x 256, NeRF-MVL-style: ground-truth ray-drop -1 outside a 24 x 200 window) with one render m0.  A render's `low`
variant has every predicted ray-drop scaled to <= 0.5.  Render k1 carries pixels at DepthMeter's clamps (0, 1e-4 m, 80 m,
100 m).  Per case and frame: eval_step's masked intensity / depth, its loss, test_step's intensity / depth; per case the
meters.  Images that repeat (a case that leaves the render unmasked, two cases that mask alike) are stored once: the case
list names the array.  With nerf_mvl eval_step returns the intensity CROPPED to the window; the full-frame `pred_intensity`
stored for those cases is the render's intensity times this script's own statement of the mask, asserted equal to the
reference's crop inside the window — outside it the reference pins the mask through the full-frame `pred_depth` only, which
it does return.  (The shared frame is 24 x 515, not 33 x 515: the file stays below 1 MiB.)  Predicted ray-drops stay 1e-3 away from 0.5 and depth ratios 1e-4 away from 1.25^k (asserted).
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCALE = 0.010784853507573345  # configs/kitti360_1908.txt:12
ALPHAS = dict(alpha_d=1000.0, alpha_r=1.0, alpha_i=10.0)
INV_SCALE = 255.0             # MAEMeter(intensity_inv_scale=) (main_lidarnerf.py:54, 362)
DEFAULT = ("l1", "mse", "mse")


def make_gt(H, W, seed, window=None):
    g = torch.Generator().manual_seed(seed)
    raydrop = (torch.rand(H, W, generator=g) < 0.8).float()
    intensity = torch.rand(H, W, generator=g)
    metres = 2.0 + 76.0 * torch.rand(H, W, generator=g)
    if window is not None:
        r0, c0, h, w = window
        inside = torch.zeros(H, W, dtype=torch.bool)
        inside[r0:r0 + h, c0:c0 + w] = True
        raydrop = torch.where(inside, raydrop, torch.tensor(-1.0))
    return torch.stack([raydrop, intensity, SCALE * metres], -1)


def make_render(gt, seed, rel, clamps=False):
    """image [H*W, 2], depth [H*W] as the renderer returns them."""
    H, W, _ = gt.shape
    g = torch.Generator().manual_seed(seed)
    kept = gt[..., 0] == 1
    raydrop = torch.where(kept, 0.55 + 0.45 * torch.rand(H, W, generator=g), 0.45 * torch.rand(H, W, generator=g))
    flip = torch.rand(H, W, generator=g) < 0.1  # a tenth of the pixels predict the wrong side
    raydrop = torch.where(flip, 1.0 - raydrop, raydrop)
    intensity = (gt[..., 1] + 0.05 * torch.randn(H, W, generator=g)).clamp(0, 1)
    depth = gt[..., 2] * (1 + rel * torch.randn(H, W, generator=g))
    depth = torch.where(kept, depth, SCALE * 60.0 * torch.rand(H, W, generator=g))  # something where the truth dropped
    if clamps:
        for c, m in enumerate((0.0, 1e-4, 80.0, 100.0)):  # as G11 plants them; kept pixels, so the mask leaves them
            depth[0, c] = SCALE * m
            raydrop[0, c] = 0.9
            gt[0, c, 0] = 1.0
    return torch.stack([raydrop, intensity], -1).reshape(H * W, 2), depth.reshape(H * W)


def check_margins(image, depth, gt, mvl, fix=False):
    """No comparison on a rounding edge; fix: move the depth of an offending pixel by 0.2 % first (the values are arbitrary)."""
    assert (image[:, 0] - 0.5).abs().min() >= 1e-3
    if fix:
        for _ in range(8):
            bad = _near_threshold(image, depth, gt, mvl)
            depth[bad] *= 1.002
        return check_margins(image, depth, gt, mvl)
    assert not _near_threshold(image, depth, gt, mvl).any()


def _near_threshold(image, depth, gt, mvl):
    H, W, _ = gt.shape
    gr = gt[..., 0].double()
    if mvl:
        gr = torch.where(gr == -1, 0.0, gr)
    G = (gt[..., 2].double() * gr / SCALE).clamp(1e-3, 80)
    bad = torch.zeros(H, W, dtype=torch.bool)
    for mask in (torch.ones(H, W), (image[:, 0] > 0.5).reshape(H, W).double()):
        P = (depth.reshape(H, W).double() * mask / SCALE).clamp(1e-3, 80)
        th = torch.maximum(G / P, P / G)
        for k in (1, 2, 3):
            bad |= ((th / 1.25 ** k) - 1).abs() < 1e-4
    return bad.reshape(-1)


def cases():
    out = []

    def add(name, frames, mvl=False, criteria=DEFAULT, **alphas):
        out.append(dict(name=name, frames=frames, nerf_mvl=mvl, criteria=list(criteria), alphas=dict(ALPHAS, **alphas)))

    add("default", ["k0"])
    add("all_low", ["k0_low"])            # eval_step's unmasked branch, test_step's masked one
    add("alpha_r0", ["k0"], alpha_r=0.0)
    add("nerf_mvl", ["m0"], mvl=True)
    add("huber_bce_l1", ["k0"], criteria=("huber", "bce", "l1"))
    add("clamps", ["k1"])
    add("two_frames", ["k0", "k1"])       # the meters average per-frame values
    add("nerf_mvl_huber", ["m0"], mvl=True, criteria=("huber", "mse", "huber"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference project")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from make_golden import _reference_trainer
    Trainer = _reference_trainer()
    import lidarnerf.nerf.utils as ref_utils
    ref_utils.structural_similarity = lambda a, b, data_range=None: float("nan")  # (scikit-image: see the docstring)
    torch.set_num_threads(4)

    window = (4, 16, 24, 200)
    gt_k, gt_m = make_gt(24, 515, 1401), make_gt(32, 256, 1402, window)
    renders = {"k0": (gt_k, *make_render(gt_k, 1411, 0.03)), "k1": (gt_k, *make_render(gt_k, 1412, 0.08, clamps=True)),
               "m0": (gt_m, *make_render(gt_m, 1413, 0.05))}
    out = {"gt_k": gt_k.numpy(), "gt_m": gt_m.numpy(), "window_m": np.array(window, dtype=np.int32)}
    for name, (gt, image, depth) in renders.items():
        check_margins(image, depth, gt, name.startswith("m"), fix=True)
        out[f"{name}_image"], out[f"{name}_depth"] = image.numpy(), depth.numpy()

    def render_of(key):
        base = key.split("_")[0]
        gt, image, depth = renders[base]
        if key.endswith("_low"):
            image = image.clone()
            image[:, 0] *= 0.49
            assert image[:, 0].max() <= 0.5 - 1e-3
        return gt, image, depth

    def store(prefix, array):
        """Name of the stored array holding `array`: an earlier one with the same bytes, or a new one."""
        a = np.ascontiguousarray(array, dtype=np.float32)
        for k, v in out.items():
            if v.dtype == np.float32 and v.size == a.size and np.array_equal(v.reshape(-1).view(np.int32), a.reshape(-1).view(np.int32)):
                return k
        out[prefix] = a
        return prefix

    all_cases = cases()
    for c in all_cases:
        opt = argparse.Namespace(enable_lidar=True, dataloader="nerf_mvl" if c["nerf_mvl"] else "kitti360", scale=SCALE,
                                 **c["alphas"])
        loss_dict = {  # main_lidarnerf.py:330-342
            "mse": torch.nn.MSELoss(reduction="none"), "l1": torch.nn.L1Loss(reduction="none"),
            "bce": torch.nn.BCEWithLogitsLoss(reduction="none"),
            "huber": torch.nn.HuberLoss(reduction="none", delta=0.2 * SCALE)}
        criterion = dict(zip(("depth", "raydrop", "intensity"), (loss_dict[k] for k in c["criteria"])))
        meters = [ref_utils.MAEMeter(intensity_inv_scale=INV_SCALE), ref_utils.RMSEMeter(), ref_utils.DepthMeter(scale=SCALE)]
        c["per_frame"] = []
        for j, key in enumerate(c["frames"]):
            gt, image, depth = render_of(key)
            H, W, _ = gt.shape

            class _Model:
                def render(self, rays_o, rays_d, **kw):
                    assert kw["cal_lidar_color"] and kw["staged"]
                    return {"image_lidar": image.clone()[None], "depth_lidar": depth.clone()[None]}

            me = types.SimpleNamespace(opt=opt, model=_Model(), criterion=criterion, device=torch.device("cpu"))
            data = {"rays_o_lidar": torch.zeros(1, H * W, 3), "rays_d_lidar": torch.zeros(1, H * W, 3),
                    "images_lidar": gt.clone()[None], "H_lidar": H, "W_lidar": W}
            with torch.no_grad():
                r = Trainer.eval_step(me, data)
                t = Trainer.test_step(me, data)
            pi, pd, pdc, pr, gi, gd, gdc, gr, loss = r
            if c["nerf_mvl"]:
                assert tuple(pdc.shape) == (1, window[2], window[3]) == tuple(gdc.shape) and pi.shape == (1, window[2], window[3], 1)
                # eval_step returns the intensity cropped: keep the full masked image for the comparison (crop x 0 / 1 rule
                # is the same; the crop is checked through the meters and the shapes recorded here)
                full = image.reshape(H, W, 2)[..., 1].clone()
                r0, c0, h, w = window
                mask_applied = not torch.equal(pd[0], depth.reshape(H, W))
                if mask_applied:
                    full = full * ((image.reshape(H, W, 2)[..., 0] > 0.5) & (gt[..., 0] != -1)).long()
                assert torch.equal(full[r0:r0 + h, c0:c0 + w], pi[0, ..., 0])
                assert torch.equal(pd[0, r0:r0 + h, c0:c0 + w], pdc[0])
                pi_full = full
            else:
                assert pdc is None and gdc is None and tuple(pi.shape) == (1, H, W, 1)
                pi_full = pi[0, ..., 0]
            assert tuple(pd.shape) == (1, H, W) and tuple(pr.shape) == (1, H, W, 1) and tuple(gr.shape) == (1, H, W, 1)
            assert all(x.shape == (1, H, W) for x in t)
            for i, meter in enumerate(meters):  # utils.py:1357-1366
                if i < 2:
                    meter.update(pi, gi)
                elif c["nerf_mvl"]:
                    meter.update(pdc, gdc)
                else:
                    meter.update(pd, gd)
            tag = f"{c['name']}_f{j}"
            rec = dict(render=key,
                       pred_intensity=store(f"{tag}_pred_intensity", pi_full.numpy()),
                       pred_depth=store(f"{tag}_pred_depth", pd[0].numpy()),
                       test_intensity=store(f"{tag}_test_intensity", t[1][0].numpy()),
                       test_depth=store(f"{tag}_test_depth", t[2][0].numpy()),
                       loss=float(loss), crop=list(pdc.shape[1:]) if pdc is not None else None,
                       depth_errors=[float(v) for v in meters[2].V[-1][:4]])
            c["per_frame"].append(rec)
            print(f"{tag:24s} loss {float(loss):.6g}  depth {rec['depth_errors']}")
        c["mae"], c["rmse"] = float(meters[0].measure()), float(meters[1].measure())
        c["depth"] = [float(v) for v in meters[2].measure()[:4]]
    out.update(cases=np.array(json.dumps(all_cases)), scale=np.float64(SCALE), intensity_inv_scale=np.float64(INV_SCALE))
    path = os.path.join(HERE, "g14_eval_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), sorted(out))
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
