"""Evaluation loop of the reference Trainer on the fast trainer (lidarnerf/nerf/utils.py:886-1009 eval_step / test_step,
1282-1447 evaluate_one_epoch): the render of a full frame, the fused frame epilogue (metrics.FrameEvaluator, csrc/
eval_frame.hip) and the bookkeeping around them.  LidarTrainer.eval_step / test_step / evaluate call into here."""
import contextlib
import os

import numpy as np
import torch

from .. import _hip

HISTORY_FRAMES = 4096  # rows of per-frame history evaluate() keeps (the means and the bad-frame count cover every frame)


def _render(trainer, rays_o, rays_d, perturb):
    with torch.no_grad(), torch.autocast("cuda", dtype=trainer.amp_dtype, enabled=trainer.fp16):
        return trainer.model.render(rays_o, rays_d, cal_lidar_color=True, staged=True, perturb=perturb,
                                    **trainer.render_kwargs)


def _frame(data):
    for key in ("rays_o_lidar", "rays_d_lidar", "images_lidar"):
        if key not in data:
            raise KeyError(f"evaluation frame without {key!r} (keys: rays_o_lidar, rays_d_lidar, images_lidar, H_lidar, W_lidar)")
        if not torch.is_tensor(data[key]) or not data[key].is_cuda:
            raise RuntimeError(f"LidarTrainer evaluation: data[{key!r}] must be a tensor on the GPU (no CPU fallback)")
    images = data["images_lidar"]
    if images.dim() != 4 or images.shape[0] != 1 or images.shape[-1] < 3:
        raise ValueError(f"images_lidar must be [1, H, W, 3] (one frame per step), got {tuple(images.shape)}")
    return data["rays_o_lidar"], data["rays_d_lidar"], images[..., :3]


def frame_evaluator(trainer, H, W, max_frames):
    from ..metrics import FrameEvaluator
    ad, ar, ai, _ = trainer.alpha
    return FrameEvaluator(H, W, trainer.scale, intensity_inv_scale=trainer.intensity_inv_scale, alphas=(ad, ar, ai),
                          loss_options=trainer.loss_options, nerf_mvl=trainer.nerf_mvl, max_frames=max_frames)


def _step_evaluator(trainer, H, W):
    """The one-row evaluator eval_step and test_step share: the trainer keeps ONE, rebuilt when the frame size or an option
    it was built from has changed."""
    key = (H, W, trainer.nerf_mvl, trainer.alpha, trainer.loss_options, trainer.scale, trainer.intensity_inv_scale)
    kept = getattr(trainer, "_step_evaluator", None)
    if kept is None or kept[0] != key:
        kept = trainer._step_evaluator = (key, frame_evaluator(trainer, H, W, 1))
    return kept[1]


def eval_step(trainer, data):
    """The reference's nine values (utils.py:967-977), shapes and dtypes included."""
    rays_o, rays_d, images = _frame(data)
    _, H, W, _ = images.shape
    ev = _step_evaluator(trainer, H, W)
    out = _render(trainer, rays_o, rays_d, False)
    ev.clear()
    pred_intensity, pred_depth, _ = ev.update(out["image_lidar"], out["depth_lidar"], images, mode="eval")
    loss = ev.state[0, 0].float()
    pred_raydrop = out["image_lidar"].float().reshape(1, H, W, 2)[..., 0]
    gt_raydrop = images[..., 0]
    if trainer.nerf_mvl:
        gt_raydrop = gt_raydrop * torch.where(gt_raydrop == -1, 0, 1)
    gt_intensity, gt_depth = images[..., 1] * gt_raydrop, images[..., 2] * gt_raydrop
    pred_intensity, pred_depth = pred_intensity[None], pred_depth[None]
    pred_depth_crop = gt_depth_crop = None
    if trainer.nerf_mvl:
        # the crop's shape is a host value: this compatibility method reads one row back (the fused loop never does)
        row = dict(zip(_hip.EVAL_SLOT_NAMES, ev.state[1].tolist()))
        r0, c0, h, w = (int(row[k]) for k in ("crop_r0", "crop_c0", "crop_h", "crop_w"))
        if int(row["valid"]) != h * w:
            raise RuntimeError(f"eval_step: shape '[1, {h}, {w}]' is invalid for input of size {int(row['valid'])} (the valid "
                               "pixels of a NeRF-MVL frame must fill their bounding rectangle)")
        crop = lambda t: t[:, r0:r0 + h, c0:c0 + w].contiguous()
        pred_intensity, gt_intensity = crop(pred_intensity), crop(gt_intensity)
        pred_depth_crop, gt_depth_crop = crop(pred_depth), crop(gt_depth)
    return (pred_intensity.unsqueeze(-1), pred_depth, pred_depth_crop, pred_raydrop.unsqueeze(-1),
            gt_intensity.unsqueeze(-1), gt_depth, gt_depth_crop, gt_raydrop.unsqueeze(-1), loss)


def test_step(trainer, data, perturb=False):
    """(pred_raydrop, pred_intensity, pred_depth), [B, H, W] each (utils.py:980-1009)."""
    for key in ("rays_o_lidar", "rays_d_lidar", "H_lidar", "W_lidar"):
        if key not in data:
            raise KeyError(f"test frame without {key!r}")
    rays_o, rays_d, H, W = data["rays_o_lidar"], data["rays_d_lidar"], int(data["H_lidar"]), int(data["W_lidar"])
    if not (torch.is_tensor(rays_o) and rays_o.is_cuda and torch.is_tensor(rays_d) and rays_d.is_cuda):
        raise RuntimeError("LidarTrainer.test_step: rays must be tensors on the GPU (no CPU fallback)")
    ev = _step_evaluator(trainer, H, W)
    out = _render(trainer, rays_o, rays_d, perturb)
    image = out["image_lidar"].float().reshape(-1, H, W, 2)
    B = image.shape[0]
    pred_intensity, pred_depth, _ = ev.mask(image, out["depth_lidar"])
    return image[..., 0], pred_intensity.reshape(B, H, W), pred_depth.reshape(B, H, W)


def evaluate(trainer, frames, *, points_intrinsics=None, ema=True, save_dir=None, fused_points=False):
    from ..metrics import FramePointsEvaluator, PointsMeter
    from ..convert import pano_to_lidar
    model = trainer.model
    was_training = model.training
    use_ema = bool(ema) and trainer.ema is not None
    ev, points, n = None, None, 0
    if points_intrinsics is not None and not fused_points:
        points = PointsMeter(trainer.scale, points_intrinsics)
    if save_dir is not None:
        if points_intrinsics is None:
            raise ValueError("evaluate(save_dir=) writes point clouds: it needs points_intrinsics")
        os.makedirs(save_dir, exist_ok=True)
    model.eval()
    try:
        with (trainer.ema_weights() if use_ema else contextlib.nullcontext()):
            for data in frames:
                rays_o, rays_d, images = _frame(data)
                _, H, W, _ = images.shape
                if ev is None:
                    ev = frame_evaluator(trainer, H, W, HISTORY_FRAMES)
                elif (ev.H, ev.W) != (H, W):
                    raise ValueError(f"evaluate: frames of one size wanted ({ev.H} x {ev.W}, then {H} x {W})")
                out = _render(trainer, rays_o, rays_d, False)
                _, pred_depth, _ = ev.update(out["image_lidar"], out["depth_lidar"], images, mode="eval")
                n += 1
                if fused_points and points_intrinsics is not None:  # (the same meter with no host read per frame)
                    if points is None:
                        points = FramePointsEvaluator(H, W, trainer.scale, points_intrinsics, nerf_mvl=trainer.nerf_mvl,
                                                      max_frames=HISTORY_FRAMES)
                    points.update(pred_depth, images)
                elif points is not None:  # (the full frame, also with nerf_mvl: utils.py:1361-1366)
                    gr = images[..., 0]
                    if trainer.nerf_mvl:
                        gr = gr * torch.where(gr == -1, 0, 1)
                    points.update(pred_depth[None], images[..., 2] * gr)
                if save_dir is not None:
                    # (the fused meter has just built this cloud; reading its row count is the one host read it costs)
                    cloud = points.cloud() if fused_points else pano_to_lidar(pred_depth / trainer.scale, points_intrinsics)
                    np.save(os.path.join(save_dir, f"ep{trainer.epoch:04d}_{n:04d}_lidar.npy"), cloud.cpu().numpy())
    finally:
        model.train(was_training)
    if ev is None:
        raise ValueError("evaluate: no frames")
    result = ev.measure()
    # utils.py:1422-1436: the result is the first number of the LAST meter
    trainer.stats["valid_loss"].append(result["loss"])
    if points is not None:
        result["points"] = points.measure()
        trainer.stats["results"].append(float(result["points"][0]))
    else:
        trainer.stats["results"].append(float(result["depth"][0]))
    return result
