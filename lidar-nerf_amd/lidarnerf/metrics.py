"""Evaluation metrics on the device: the meters of lidarnerf/nerf/utils.py:226-427 that the LiDAR
evaluation uses, without the reference's round trip through NumPy/CPU, and the chamfer distance of
extern/chamfer3D (dist_chamfer_3D.py, chamfer3D.cu) + extern/fscore.py on the HIP nearest-neighbour kernel.

Same class names, constructor arguments, `update / measure / report / clear` protocol and numbers; inputs are CUDA
tensors (NumPy arrays are moved to the GPU).  Not here: PSNR/LPIPS image meters of the RGB branch.

FrameEvaluator is the fused form of what Trainer.eval_step / test_step do after the render plus the MAE / RMSE / Depth
meters (csrc/eval_frame.hip): four launches per frame, no host read until measure().
"""
import ctypes as C

import numpy as np
import torch

from . import _hip
from .convert import pano_to_lidar


def _gpu(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    return x.detach().cuda().float()


class chamfer_3DDist(torch.nn.Module):
    """dist1 [B,n], dist2 [B,m] squared nearest-neighbour distances, idx1 / idx2 int32 (dist_chamfer_3D.py:37-84).
    Forward only (the reference's evaluation never back-propagates through it)."""

    def forward(self, xyz1, xyz2):
        xyz1, xyz2 = xyz1.float().contiguous(), xyz2.float().contiguous()
        if not (xyz1.is_cuda and xyz2.is_cuda):
            raise RuntimeError("chamfer_3DDist: inputs must live on the GPU (no CPU fallback)")
        B, n, d1 = xyz1.shape
        _, m, d2 = xyz2.shape
        assert d1 == 3 and d2 == 3, "Wrong last dimension for the chamfer distance 's input! Check with .size()"
        dist1 = torch.zeros((B, n), device=xyz1.device)
        dist2 = torch.zeros((B, m), device=xyz1.device)
        idx1 = torch.zeros((B, n), dtype=torch.int32, device=xyz1.device)
        idx2 = torch.zeros((B, m), dtype=torch.int32, device=xyz1.device)
        for b in range(B):
            _hip.call("lnh_chamfer_nn", xyz1[b].data_ptr(), n, xyz2[b].data_ptr(), m, dist1[b].data_ptr(),
                      idx1[b].data_ptr())
            _hip.call("lnh_chamfer_nn", xyz2[b].data_ptr(), m, xyz1[b].data_ptr(), n, dist2[b].data_ptr(),
                      idx2[b].data_ptr())
        return dist1, dist2, idx1, idx2


def fscore(dist1, dist2, threshold=0.001):
    """extern/fscore.py:4-18 (distances are squared: adapt the threshold)."""
    precision_1 = torch.mean((dist1 < threshold).float(), dim=1)
    precision_2 = torch.mean((dist2 < threshold).float(), dim=1)
    f = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    f[torch.isnan(f)] = 0
    return f, precision_1, precision_2


class _Meter:
    def __init__(self):
        self.V, self.N = 0, 0

    def clear(self):
        self.V, self.N = 0, 0

    def measure(self):
        return self.V / self.N


class RMSEMeter(_Meter):
    """utils.py:226-260"""

    def update(self, preds, truths):
        preds, truths = _gpu(preds), _gpu(truths)
        self.V += float(torch.sqrt(((truths - preds) ** 2).mean()))
        self.N += 1

    def report(self):
        return f"RMSE = {self.measure():.6f}"


class MAEMeter(_Meter):
    """utils.py:263-301"""

    def __init__(self, intensity_inv_scale=1.0):
        super().__init__()
        self.intensity_inv_scale = intensity_inv_scale

    def update(self, preds, truths):
        preds, truths = _gpu(preds), _gpu(truths)
        self.V += float((truths * self.intensity_inv_scale - preds * self.intensity_inv_scale).abs().mean())
        self.N += 1

    def report(self):
        return f"MAE = {self.measure():.6f}"


def structural_similarity(im1, im2, data_range, win_size=7, K1=0.01, K2=0.03):
    """Mean SSIM with the defaults the reference relies on (skimage.metrics.structural_similarity: uniform 7x7 window,
    sample covariance, mean over the region the window covers completely)."""
    x, y = im1[None, None].double(), im2[None, None].double()
    pool = torch.nn.functional.avg_pool2d
    ux, uy = pool(x, win_size, 1), pool(y, win_size, 1)
    uxx, uyy, uxy = pool(x * x, win_size, 1), pool(y * y, win_size, 1), pool(x * y, win_size, 1)
    norm = win_size ** 2 / (win_size ** 2 - 1.0)
    vx, vy, vxy = norm * (uxx - ux * ux), norm * (uyy - uy * uy), norm * (uxy - ux * uy)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float(s.mean())


class DepthMeter:
    """utils.py:304-362: (rmse, a1, a2, a3, ssim) of a [1,H,W] depth image in metres."""

    def __init__(self, scale):
        self.V, self.N, self.scale = [], 0, scale

    def clear(self):
        self.V, self.N = [], 0

    def update(self, preds, truths):
        preds, truths = _gpu(preds) / self.scale, _gpu(truths) / self.scale
        self.V.append(list(self.compute_depth_errors(truths, preds)))
        self.N += 1

    def compute_depth_errors(self, gt, pred, min_depth=1e-3, max_depth=80, thresh_set=1.25):
        pred, gt = pred.clamp(min_depth, max_depth), gt.clamp(min_depth, max_depth)
        thresh = torch.maximum(gt / pred, pred / gt)
        a1 = float((thresh < thresh_set).float().mean())
        a2 = float((thresh < thresh_set ** 2).float().mean())
        a3 = float((thresh < thresh_set ** 3).float().mean())
        rmse = float(torch.sqrt(((gt - pred) ** 2).mean()))
        ssim = structural_similarity(pred.squeeze(0), gt.squeeze(0), data_range=float(gt.max() - gt.min()))
        return rmse, a1, a2, a3, ssim

    def measure(self):
        assert self.N == len(self.V)
        return np.array(self.V).mean(0)

    def report(self):
        return f"Depth_error(rmse, a1, a2, a3, ssim) = {self.measure()}"


class PointsMeter:
    """utils.py:365-413: chamfer distance + F-score (threshold 0.05 on squared distances) of the point clouds
    back-projected from the predicted and the ground-truth range image."""

    def __init__(self, scale, intrinsics):
        self.V, self.N, self.scale, self.intrinsics = [], 0, scale, intrinsics

    def clear(self):
        self.V, self.N = [], 0

    def update(self, preds, truths):
        preds, truths = _gpu(preds) / self.scale, _gpu(truths) / self.scale
        pred_lidar = pano_to_lidar(preds[0], self.intrinsics)
        gt_lidar = pano_to_lidar(truths[0], self.intrinsics)
        dist1, dist2, _, _ = chamfer_3DDist()(pred_lidar[None], gt_lidar[None])
        chamfer_dis = dist1.mean() + dist2.mean()
        f, _, _ = fscore(dist1, dist2, 0.05)
        self.V.append([float(chamfer_dis), float(f[0])])
        self.N += 1

    def measure(self):
        assert self.N == len(self.V)
        return np.array(self.V).mean(0)

    def report(self):
        return f"CD f-score = {self.measure()}"


class FrameEvaluator:
    """The evaluation epilogue of a LiDAR frame on the device (lnh_lidar_eval_frame / _ssim / _finalize, include/
    lidarnerf_hip.h): the ray-drop masking of the reference's eval_step / test_step (utils.py:886-1009), its validation
    loss, and the numbers its MAEMeter, RMSEMeter and DepthMeter would report for the frame (utils.py:1357-1366), added to a
    running accumulator on the device.  Meters average per-frame values, as the reference's do.

        ev = FrameEvaluator(H, W, scale)
        for frame in frames:
            pred_intensity, pred_depth, mask = ev.update(out["image_lidar"], out["depth_lidar"], gt)   # no host read
        numbers = ev.measure()                                                                          # ONE copy to the host

    alphas = (alpha_d, alpha_r, alpha_i); loss_options: a nerf.loss.LidarLossOptions (its three per-ray criteria;
    huber's delta is 0.2 * scale); nerf_mvl: ground-truth ray-drop -1 marks pixels outside the sensor's window; max_frames:
    rows of per-frame history kept (later frames still count in the means).  update() allocates its three output images
    and nothing else after the first call, and never synchronises: it can be captured in a torch.cuda.graph after one
    eager call.  SSIM restates skimage's defaults (see structural_similarity above).  No CPU fallback."""

    def __init__(self, H, W, scale, intensity_inv_scale=1.0, alphas=(1000.0, 1.0, 10.0), loss_options=None, nerf_mvl=False,
                 max_frames=1024):
        from .nerf.loss import LidarLossOptions
        self.H, self.W, self.scale = int(H), int(W), float(scale)
        if self.H < 1 or self.W < 1:
            raise ValueError(f"FrameEvaluator: H ({H}) and W ({W}) must be positive")
        if not self.scale > 0:
            raise ValueError("FrameEvaluator: scale must be positive")
        self.intensity_inv_scale, self.nerf_mvl, self.max_frames = float(intensity_inv_scale), bool(nerf_mvl), int(max_frames)
        if self.max_frames < 0:
            raise ValueError("FrameEvaluator: max_frames must not be negative")
        self.alphas = tuple(float(a) for a in alphas)
        if len(self.alphas) != 3:
            raise ValueError("FrameEvaluator: alphas = (alpha_d, alpha_r, alpha_i)")
        self.loss_options = loss_options if loss_options is not None else LidarLossOptions()
        if not isinstance(self.loss_options, LidarLossOptions):
            raise TypeError(f"FrameEvaluator(loss_options=): a LidarLossOptions, not {type(self.loss_options).__name__}")
        self._opt = _hip.loss_options(self.loss_options, 1, 1, self.scale, self.loss_options.huber_delta(self.scale),
                                      *self.alphas, 0.0)
        self.state = self._ws = None  # [1 + max_frames, EVAL_SLOTS] f64: row 0 the accumulator, then the history

    def _alloc(self, device):
        _hip.require_symbols(("lnh_lidar_eval_frame", "lnh_lidar_eval_ssim", "lnh_lidar_eval_finalize",
                              "lnh_lidar_eval_workspace_bytes"), "metrics.FrameEvaluator")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FrameEvaluator: call update() once eagerly before capturing it (its buffers must exist)")
        nbytes = int(_hip.lib().lnh_lidar_eval_workspace_bytes(self.H, self.W))
        self._ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)
        self.state = torch.zeros((1 + self.max_frames, _hip.EVAL_SLOTS), dtype=torch.float64, device=device)

    def clear(self):
        if self.state is not None:
            self.state.zero_()

    def update(self, image_lidar, depth_lidar, images_lidar, mode="eval"):
        """image_lidar [.., H*W, 2], depth_lidar [.., H*W] (the renderer's outputs for ONE frame), images_lidar [.., H, W, 3]
        ground truth; mode "eval" / "test": whose masking rule.  Returns (pred_intensity, pred_depth, mask), [H, W] f32 each:
        the masked prediction images and the thresholded ray-drop mask (1.0 / 0.0)."""
        if mode not in _hip.EVAL_MODES:
            raise ValueError(f"FrameEvaluator.update: mode {mode!r} is not 'eval' or 'test'")
        if self.H < 7 or self.W < 7:  # (mask(), test_step's rule without a ground truth, has no such limit)
            raise ValueError(f"FrameEvaluator.update: H ({self.H}) and W ({self.W}) must be at least 7 (the SSIM window)")
        for name, t in (("image_lidar", image_lidar), ("depth_lidar", depth_lidar), ("images_lidar", images_lidar)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"FrameEvaluator.update: {name} must be a tensor on the GPU (no CPU fallback)")
        N = self.H * self.W
        if image_lidar.numel() != 2 * N or depth_lidar.numel() != N or images_lidar.numel() != 3 * N:
            raise ValueError(f"FrameEvaluator.update: one {self.H} x {self.W} frame wanted (image_lidar [{N}, 2], depth_lidar "
                             f"[{N}], images_lidar [{self.H}, {self.W}, 3]), got {tuple(image_lidar.shape)}, "
                             f"{tuple(depth_lidar.shape)}, {tuple(images_lidar.shape)}")
        image, depth, gt = (t.detach().float().contiguous() for t in (image_lidar, depth_lidar, images_lidar))
        if self.state is None:
            self._alloc(image.device)
        out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=image.device)
        opt, code, mvl = C.cast(C.pointer(self._opt), C.c_void_p), _hip.EVAL_MODES[mode], int(self.nerf_mvl)
        ws, ws_bytes = self._ws.data_ptr(), self._ws.numel() * 8
        _hip.call("lnh_lidar_eval_frame", image.data_ptr(), depth.data_ptr(), gt.data_ptr(), self.H, self.W, opt,
                  self.intensity_inv_scale, code, mvl, ws, ws_bytes, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        _hip.call("lnh_lidar_eval_ssim", out[1].data_ptr(), gt.data_ptr(), self.H, self.W, self.scale, mvl, ws, ws_bytes)
        _hip.call("lnh_lidar_eval_finalize", self.H, self.W, opt, code, mvl, ws, ws_bytes, self.state.data_ptr(),
                  self.state[1:].data_ptr() if self.max_frames else None, self.max_frames)
        return out[0], out[1], out[2]

    def mask(self, image_lidar, depth_lidar):
        """test_step's masking without a ground truth (utils.py:998-1007) on any number of rows of width W: image_lidar
        [.., 2], depth_lidar [..] -> (pred_intensity, pred_depth, mask) [rows, W].  Nothing is accumulated."""
        for name, t in (("image_lidar", image_lidar), ("depth_lidar", depth_lidar)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"FrameEvaluator.mask: {name} must be a tensor on the GPU (no CPU fallback)")
        n = depth_lidar.numel()
        if n == 0 or n % self.W or image_lidar.numel() != 2 * n:
            raise ValueError(f"FrameEvaluator.mask: rows of {self.W} pixels wanted, got {tuple(image_lidar.shape)}, "
                             f"{tuple(depth_lidar.shape)}")
        _hip.require_symbols(("lnh_lidar_eval_frame",), "metrics.FrameEvaluator")
        image, depth = image_lidar.detach().float().contiguous(), depth_lidar.detach().float().contiguous()
        out = torch.empty((3, n // self.W, self.W), dtype=torch.float32, device=image.device)
        _hip.call("lnh_lidar_eval_frame", image.data_ptr(), depth.data_ptr(), None, n // self.W, self.W,
                  C.cast(C.pointer(self._opt), C.c_void_p), self.intensity_inv_scale, _hip.EVAL_MODES["test"], 0, None, 0,
                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        return out[0], out[1], out[2]

    def measure(self):
        """One device-to-host copy.  {"frames", "loss", "mae", "rmse", "depth": array (rmse, a1, a2, a3, ssim), "history":
        {slot name: per-frame array}} — means over the frames of the per-frame values.  Refuses (RuntimeError naming the
        frame) an evaluation with a frame whose numbers cannot be averaged: NeRF-MVL valid pixels that do not fill their
        rectangle, or a non-finite number."""
        if self.state is None:
            raise RuntimeError("FrameEvaluator.measure: no frame has been evaluated")
        host = self.state.cpu().numpy()
        acc, n = host[0], int(host[0][_hip.EVAL_SLOT_NAMES.index("frames")])
        if n == 0:
            raise RuntimeError("FrameEvaluator.measure: no frame has been evaluated")
        rows = host[1:1 + min(n, self.max_frames)]
        hist = {name: rows[:, k].copy() for k, name in enumerate(_hip.EVAL_SLOT_NAMES) if name != "frames"}
        n_bad = int(acc[_hip.EVAL_SLOT_NAMES.index("bad")])
        if n_bad:
            # a row the means cannot use (the kernel counts them, also beyond the history): valid pixels that do not fill
            # their rectangle — the reference's reshape to [B, crop_h, crop_w] raises there, utils.py:949-956 — or a
            # non-finite number (no valid pixel, a window below 7 x 7, a non-finite render)
            bad = np.nonzero(hist["bad"])[0]
            where = f"frame {int(bad[0])}" if bad.size else f"a frame beyond the {self.max_frames} kept in the history"
            why = ""
            if bad.size:
                k = int(bad[0])
                if hist["valid"][k] != hist["crop_h"][k] * hist["crop_w"][k]:
                    why = (f": the {int(hist['valid'][k])} valid pixels do not fill their {int(hist['crop_h'][k])} x "
                           f"{int(hist['crop_w'][k])} bounding rectangle")
                else:
                    why = ": " + ", ".join(f"{name} = {hist[name][k]}" for name in _hip.EVAL_SLOT_NAMES[:11]
                                           if not np.isfinite(hist[name][k])) + \
                          f" ({int(hist['valid'][k])} valid pixels, window {int(hist['crop_h'][k])} x {int(hist['crop_w'][k])})"
            raise RuntimeError(f"FrameEvaluator.measure: {n_bad} of {n} frames cannot be averaged; {where}{why}")
        mean = {name: acc[k] / n for k, name in enumerate(_hip.EVAL_SLOT_NAMES)}
        return {"frames": n, "loss": float(mean["loss"]), "mae": float(mean["mae"]), "rmse": float(mean["rmse"]),
                "depth": np.array([mean["depth_rmse"], mean["a1"], mean["a2"], mean["a3"], mean["ssim"]]), "history": hist}

    def report(self):
        """The three lines the reference's meters log (utils.py:262, 304, 372)."""
        m = self.measure()
        text = f"MAE = {m['mae']:.6f}\nRMSE = {m['rmse']:.6f}\nDepth_error(rmse, a1, a2, a3, ssim) = {m['depth']}"
        print(text)
        return text


class FramePointsEvaluator:
    """The points meter of a LiDAR frame on the device (lnh_eval_points_project / _nn / _finalize, include/lidarnerf_hip.h,
    csrc/eval_points.hip): what PointsMeter computes — both depth images back-projected to point clouds, the chamfer
    distance and the F-score between them — from the masked predicted depth FrameEvaluator.update returns and the ground-
    truth frame to a row of numbers in an accumulator on the device.

        pts = FramePointsEvaluator(H, W, scale, (fov_up, fov))
        for frame in frames:
            pts.update(pred_depth, images_lidar)          # no host read
        chamfer, fscore = pts.measure()                    # ONE copy to the host

    threshold: the F-score's, on SQUARED distances (PointsMeter's 0.05); nerf_mvl: ground-truth ray-drop -1 counts as 0;
    max_frames: rows of per-frame history kept (later frames still count in the means).  update() allocates on its first
    call only and never synchronises: it can be captured in a torch.cuda.graph after one eager call.  The clouds equal
    convert.pano_to_lidar(depth / scale, intrinsics) bit for bit, the distances lnh_chamfer_nn's; per-frame means are taken
    in fp64 (PointsMeter: fp32).  No CPU fallback."""

    def __init__(self, H, W, scale, intrinsics, threshold=0.05, nerf_mvl=False, max_frames=1024):
        self.H, self.W, self.scale = int(H), int(W), float(scale)
        if self.H < 1 or self.W < 1:
            raise ValueError(f"FramePointsEvaluator: H ({H}) and W ({W}) must be positive")
        if not self.scale > 0:
            raise ValueError("FramePointsEvaluator: scale must be positive")
        self.intrinsics = (float(intrinsics[0]), float(intrinsics[1]))
        self.threshold, self.nerf_mvl, self.max_frames = float(threshold), bool(nerf_mvl), int(max_frames)
        if not self.threshold > 0:
            raise ValueError("FramePointsEvaluator: threshold must be positive")
        if self.max_frames < 0:
            raise ValueError("FramePointsEvaluator: max_frames must not be negative")
        self.state = self._ws = None  # [1 + max_frames, PTS_SLOTS] f64: row 0 the accumulator, then the history

    def _alloc(self, device):
        _hip.require_symbols(("lnh_eval_points_project", "lnh_eval_points_nn", "lnh_eval_points_finalize",
                              "lnh_eval_points_workspace_bytes"), "metrics.FramePointsEvaluator")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FramePointsEvaluator: call update() once eagerly before capturing it (its buffers must exist)")
        nbytes = int(_hip.lib().lnh_eval_points_workspace_bytes(self.H, self.W))
        if nbytes == 0:
            raise ValueError(f"FramePointsEvaluator: a frame of {self.H} x {self.W} pixels is not supported (at most 2^24)")
        cap = self.H * self.W
        self._ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)
        self.clouds = torch.zeros((2, cap, 4), dtype=torch.float32, device=device)  # predicted, ground truth: x, y, z, 0
        self.counts = torch.zeros(4, dtype=torch.int32, device=device)
        self.dist = torch.zeros((2, cap), dtype=torch.float32, device=device)
        self.idx = torch.zeros((2, cap), dtype=torch.int32, device=device)
        self.state = torch.zeros((1 + self.max_frames, _hip.PTS_SLOTS), dtype=torch.float64, device=device)

    def clear(self):
        if self.state is not None:
            self.state.zero_()

    def update(self, pred_depth, images_lidar):
        """pred_depth [.., H, W]: the masked predicted depth of ONE frame (FrameEvaluator.update's second value);
        images_lidar [.., H, W, 3]: the ground truth (ray-drop, intensity, depth).  Returns nothing."""
        for name, t in (("pred_depth", pred_depth), ("images_lidar", images_lidar)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"FramePointsEvaluator.update: {name} must be a tensor on the GPU (no CPU fallback)")
        N = self.H * self.W
        if pred_depth.numel() != N or images_lidar.numel() != 3 * N:
            raise ValueError(f"FramePointsEvaluator.update: one {self.H} x {self.W} frame wanted (pred_depth [{self.H}, {self.W}], "
                             f"images_lidar [{self.H}, {self.W}, 3]), got {tuple(pred_depth.shape)}, {tuple(images_lidar.shape)}")
        depth, gt = pred_depth.detach().float().contiguous(), images_lidar.detach().float().contiguous()
        if self.state is None:
            self._alloc(depth.device)
        self._project(depth, gt)
        self._search()

    def _project(self, depth, gt):
        """The first of update()'s two halves: both images back-projected into self.clouds, their lengths into self.counts."""
        _hip.call("lnh_eval_points_project", depth.data_ptr(), gt.data_ptr(), self.H, self.W, self.intrinsics[0],
                  self.intrinsics[1], self.scale, int(self.nerf_mvl), self._ws.data_ptr(), self._ws.numel() * 8,
                  self.clouds[0].data_ptr(), self.clouds[1].data_ptr(), self.counts.data_ptr())

    def _search(self):
        """The second half: nearest neighbours between self.clouds[0] and [1] (self.counts points each), the frame's row."""
        N, ws, ws_bytes = self.H * self.W, self._ws.data_ptr(), self._ws.numel() * 8
        _hip.call("lnh_eval_points_nn", self.clouds[0].data_ptr(), self.clouds[1].data_ptr(), self.counts.data_ptr(), N, ws,
                  ws_bytes, self.dist[0].data_ptr(), self.idx[0].data_ptr(), self.dist[1].data_ptr(), self.idx[1].data_ptr())
        _hip.call("lnh_eval_points_finalize", self.dist[0].data_ptr(), self.dist[1].data_ptr(), self.counts.data_ptr(), N,
                  self.threshold, self.state.data_ptr(), self.state[1:].data_ptr() if self.max_frames else None,
                  self.max_frames)

    def cloud(self):
        """The predicted cloud of the last frame, [count, 3] on the device (a view of the evaluator's buffer: the next
        update() overwrites it).  The one method that reads the count back."""
        if self.state is None:
            raise RuntimeError("FramePointsEvaluator.cloud: no frame has been evaluated")
        return self.clouds[0, :int(self.counts[0]), :3]

    def rows(self):
        """One device-to-host copy: (accumulator row, history rows of the frames kept), fp64, slots _hip.PTS_SLOT_NAMES."""
        if self.state is None:
            raise RuntimeError("FramePointsEvaluator.measure: no frame has been evaluated")
        host = self.state.cpu().numpy()
        n = int(host[0][_hip.PTS_SLOT_NAMES.index("frames")])
        return host[0], host[1:1 + min(n, self.max_frames)]

    def measure(self):
        """np.array([chamfer distance, F-score]): means over the frames of the per-frame values, as PointsMeter.measure().
        Refuses (RuntimeError naming the frame) an evaluation with a frame that has no chamfer distance: an empty cloud on
        either side, or a non-finite distance."""
        acc, rows = self.rows()
        slot = _hip.PTS_SLOT_NAMES.index
        n = int(acc[slot("frames")])
        if n == 0:
            raise RuntimeError("FramePointsEvaluator.measure: no frame has been evaluated")
        n_bad = int(acc[slot("bad")])
        if n_bad:
            bad = np.nonzero(rows[:, slot("bad")])[0]
            where = f"a frame beyond the {self.max_frames} kept in the history"
            if bad.size:
                k = int(bad[0])
                where = (f"frame {k}: {int(rows[k, slot('count_pred')])} predicted and {int(rows[k, slot('count_gt')])} "
                         f"ground-truth points, chamfer = {rows[k, slot('chamfer')]}")
            raise RuntimeError(f"FramePointsEvaluator.measure: {n_bad} of {n} frames have no chamfer distance; {where}")
        return np.array([acc[slot("chamfer")] / n, acc[slot("fscore")] / n])

    def report(self):
        return f"CD f-score = {self.measure()}"
