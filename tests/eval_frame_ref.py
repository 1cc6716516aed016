"""NumPy restatement of the reference's evaluation of one LiDAR frame (lidarnerf/nerf/utils.py): the masking and the loss of
Trainer.eval_step (886-977) and test_step (980-1009), and MAEMeter / RMSEMeter / DepthMeter's first four numbers (226-362)
fed as evaluate_one_epoch feeds them (1357-1366).  float32 where the reference computes in float32.  Pinned against the
reference's own code by tests/golden/g14_eval_step.npz (tests/test_g14_eval_cpu.py); the HIP kernels of csrc/eval_frame.hip
are compared with the same fixture in tests/test_eval_frame_gpu.py."""
import numpy as np

F = np.float32


def criterion(name, x, y, scale):
    """main_lidarnerf.py:330-342's loss_dict entry, reduction 'none'."""
    x, y = x.astype(F), y.astype(F)
    d = x - y
    if name == "l1":
        return np.abs(d)
    if name == "mse":
        return d * d
    if name == "huber":
        delta = F(0.2 * scale)
        a = np.abs(d)
        return np.where(a < delta, F(0.5) * d * d, delta * (a - F(0.5) * delta)).astype(F)
    if name == "bce":
        return ((F(1) - y) * x - (np.minimum(x, F(0)) - np.log1p(np.exp(-np.abs(x))))).astype(F)
    raise ValueError(name)


def valid_window(gt_raydrop):
    """(r0, c0, h, w) of the pixels whose ground-truth ray-drop is not -1, and their number."""
    rows, cols = np.nonzero(gt_raydrop != -1)
    return (int(rows.min()), int(cols.min()), int(rows.max() - rows.min() + 1), int(cols.max() - cols.min() + 1)), rows.size


def eval_step(image, depth, gt, *, alphas, scale, criteria=("l1", "mse", "mse"), nerf_mvl=False):
    """image [H*W, 2], depth [H*W], gt [H, W, 3] -> dict of eval_step's returned images ([H, W], crops [h, w] or None), the
    thresholded mask, whether it was applied, and the loss."""
    H, W, _ = gt.shape
    gt_raydrop = gt[..., 0].astype(F)
    valid = np.ones((H, W), dtype=bool)
    if nerf_mvl:
        valid = gt_raydrop != -1
        gt_raydrop = gt_raydrop * valid.astype(F)
    gt_intensity, gt_depth = gt[..., 1] * gt_raydrop, gt[..., 2] * gt_raydrop
    pred = image.reshape(H, W, 2).astype(F)
    pred_raydrop, pred_intensity, pred_depth = pred[..., 0], pred[..., 1], depth.reshape(H, W).astype(F)
    mask = (pred_raydrop > 0.5) & valid
    applied = alphas[1] > 0 and bool(mask.any())
    if applied:
        pred_intensity, pred_depth = pred_intensity * mask.astype(F), pred_depth * mask.astype(F)
    terms = [criterion(criteria[0], pred_depth, gt_depth, scale).mean(dtype=np.float64),
             criterion(criteria[1], pred_raydrop, gt_raydrop, scale).mean(dtype=np.float64),
             criterion(criteria[2], pred_intensity, gt_intensity, scale).mean(dtype=np.float64)]
    loss = alphas[0] * terms[0] + alphas[1] * terms[1] + alphas[2] * terms[2]
    out = dict(pred_intensity=pred_intensity, pred_depth=pred_depth, pred_raydrop=pred_raydrop, gt_intensity=gt_intensity,
               gt_depth=gt_depth, gt_raydrop=gt_raydrop, mask=mask.astype(F), applied=applied, loss=float(loss), terms=terms,
               pred_depth_crop=None, gt_depth_crop=None, meter_intensity=(pred_intensity, gt_intensity),
               meter_depth=(pred_depth, gt_depth))
    if nerf_mvl:
        (r0, c0, h, w), n = valid_window(gt[..., 0])
        if n != h * w:
            raise ValueError(f"shape [{h}, {w}] is invalid for input of size {n}")
        crop = lambda a: a[r0:r0 + h, c0:c0 + w]
        out.update(pred_depth_crop=crop(pred_depth), gt_depth_crop=crop(gt_depth), window=(r0, c0, h, w),
                   meter_intensity=(crop(pred_intensity), crop(gt_intensity)),
                   meter_depth=(crop(pred_depth), crop(gt_depth)))
    return out


def test_step(image, depth, H, W, *, alpha_r):
    """-> (pred_raydrop, pred_intensity, pred_depth), [H, W] each."""
    pred = image.reshape(H, W, 2).astype(F)
    pred_raydrop, pred_intensity, pred_depth = pred[..., 0], pred[..., 1], depth.reshape(H, W).astype(F)
    if alpha_r > 0:
        mask = (pred_raydrop > 0.5).astype(F)
        pred_intensity, pred_depth = pred_intensity * mask, pred_depth * mask
    return pred_raydrop, pred_intensity, pred_depth


test_step.__test__ = False  # (not a pytest test)


def clamp_metres(x, scale):
    return np.clip(x.astype(F) / F(scale), F(1e-3), F(80.0))


def frame_meters(step, *, scale, intensity_inv_scale=1.0):
    """(mae, rmse, [depth rmse, a1, a2, a3]) of one frame from eval_step's dict."""
    pi, gi = step["meter_intensity"]
    mae = np.abs(gi * F(intensity_inv_scale) - pi * F(intensity_inv_scale)).mean(dtype=np.float64)
    rmse = np.sqrt(((gi - pi) ** 2).mean(dtype=np.float64))
    pd, gd = step["meter_depth"]
    P, G = clamp_metres(pd, scale), clamp_metres(gd, scale)
    th = np.maximum(G / P, P / G)
    return float(mae), float(rmse), [float(np.sqrt(((G - P) ** 2).mean(dtype=np.float64))), float((th < 1.25).mean()),
                                     float((th < 1.25 ** 2).mean()), float((th < 1.25 ** 3).mean())]
