"""Evaluation of the NVS baselines on the device: the meters of lidarnvs/eval.py:9-135 (eval_points_and_pano) and the loop of
lidarnvs/run.py:186-244 around them (csrc/eval_nvs.hip, include/lidarnerf_hip.h: lnh_nvs_eval_*).

These are NOT the trainer's meters (metrics.FrameEvaluator / FramePointsEvaluator, nerf/utils.py): eval.py takes images in world
scale and flattens them first, so its SSIM is 1-D with a 7-wide window over the row-major sequence; dropped pixels (depth 0) take
part in the depth metrics, clamped to 1e-3; nothing is masked by a predicted ray-drop; and for NeRF-MVL both intensity images are
multiplied by 255 and all four images are cropped to the window's pixels in row-major order.  The point metrics are the points
meter's (chamfer = mean(d_pred) + mean(d_gt), extern/fscore.py at 0.05 on squared distances) on the full, uncropped clouds.

    metrics, ev = evaluate_nvs(nvs, test_frames)        # nvs: MeshNVS, PointCloudNVS or FieldNVS(trainer, scale)
    ev.report()

Unpinned against a real scikit-image build (it is not installed here): the SSIM restates skimage's published defaults, with the
window moments and S in fp64; per-frame means are fp64 sums where eval.py's np.mean of a float32 array is float32.  No CPU
fallback."""
import contextlib

import numpy as np
import torch

from . import _hip
from .metrics import FramePointsEvaluator

METRICS = _hip.NVS_METRICS
_SLOT = {name: k for k, name in enumerate(_hip.NVS_SLOT_NAMES)}


def _image(x, H, W, what, device=None):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(device)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"NVSFrameEvaluator.update: {what} must be a tensor on the GPU or a NumPy array (no CPU fallback)")
    if x.numel() != H * W:
        raise ValueError(f"NVSFrameEvaluator.update: {what} must be [{H}, {W}], got {tuple(x.shape)}")
    return x.detach().float().contiguous().reshape(H, W)


def _cloud(x, what, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(device)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError(f"NVSFrameEvaluator.update: {what} must be a tensor on the GPU or a NumPy array (no CPU fallback)")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"NVSFrameEvaluator.update: {what} must be [M, 3], got {tuple(x.shape)}")
    return x.detach().float()


class NVSFrameEvaluator:
    """eval_points_and_pano of one frame after another on the device (lnh_nvs_eval_frame / _ssim / _finalize and the points
    meter's kernels), accumulated there; means of per-frame values, as run.py:238-244 forms them.

        ev = NVSFrameEvaluator(H, W, lidar_K)
        for gt_frame in frames:
            ev.update(gt_frame, nvs.predict_frame_with_raydrop(...))     # no host read
        metrics = ev.measure()                                           # ONE copy to the host

    intrinsics: (fov_up, fov), for the back-projection of the panos (None when both sides always bring their clouds);
    nerf_mvl: crop to gt_frame["pano_mask"] and multiply both intensity images by 255 (run.py:200-217); threshold: the
    F-score's, on squared distances; max_frames: rows of per-frame history kept (later frames still count in the means);
    points_capacity: room of the cloud buffers when clouds are passed that may hold more than H * W points.  update()
    allocates on its first call only and never synchronises: after one eager call it can be captured in a torch.cuda.graph."""

    def __init__(self, H, W, intrinsics, nerf_mvl=False, threshold=0.05, max_frames=1024, points_capacity=None):
        self.H, self.W = int(H), int(W)
        if self.H < 1 or self.W < 1:
            raise ValueError(f"NVSFrameEvaluator: H ({H}) and W ({W}) must be positive")
        self.nerf_mvl, self.max_frames = bool(nerf_mvl), int(max_frames)
        if self.max_frames < 0:
            raise ValueError("NVSFrameEvaluator: max_frames must not be negative")
        self.intensity_scale = 255.0 if self.nerf_mvl else 1.0
        self.intrinsics = None if intrinsics is None else (float(intrinsics[0]), float(intrinsics[1]))
        cap = self.H * self.W if points_capacity is None else int(points_capacity)
        if cap < 1:
            raise ValueError("NVSFrameEvaluator: points_capacity must be positive")
        # the points meter at scale 1 with one row of history: its accumulator is cleared before every frame, so that row is
        # the frame's, at an address that does not move
        shape = (self.H, self.W) if points_capacity is None else (1, cap)
        self.points = FramePointsEvaluator(shape[0], shape[1], 1.0, self.intrinsics or (0.0, 1.0), threshold=threshold,
                                           nerf_mvl=False, max_frames=1)
        self._projects = points_capacity is None
        self.state = self._ws = self._mask = self._gt3 = None  # state [1 + max_frames, NVS_SLOTS] f64: accumulator, history

    def _alloc(self, device):
        _hip.require_symbols(("lnh_nvs_eval_frame", "lnh_nvs_eval_ssim", "lnh_nvs_eval_finalize",
                              "lnh_nvs_eval_workspace_bytes"), "nvs_eval.NVSFrameEvaluator")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("NVSFrameEvaluator: call update() once eagerly before capturing it (its buffers must exist)")
        nbytes = int(_hip.lib().lnh_nvs_eval_workspace_bytes(self.H, self.W))
        if nbytes == 0:
            raise ValueError(f"NVSFrameEvaluator: a frame of {self.H} x {self.W} pixels is not supported (at most 2^24)")
        self.points._alloc(device)
        self._ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)
        self._mask = torch.zeros((self.H, self.W), dtype=torch.uint8, device=device)
        self._gt3 = torch.zeros((self.H, self.W, 3), dtype=torch.float32, device=device)  # the points meter's ground truth:
        self._gt3[..., 0] = 1.0                                                          # ray-drop 1, intensity unused, depth
        self.state = torch.zeros((1 + self.max_frames, _hip.NVS_SLOTS), dtype=torch.float64, device=device)

    def clear(self):
        if self.state is not None:
            self.state.zero_()

    def _set_cloud(self, side, cloud, what):
        pts = self.points
        cloud = _cloud(cloud, what, pts.clouds.device)
        m = cloud.shape[0]
        if m > pts.clouds.shape[1]:
            raise ValueError(f"NVSFrameEvaluator.update: {what} holds {m} points, the buffers {pts.clouds.shape[1]} "
                             "(points_capacity)")
        pts.clouds[side, :m, :3].copy_(cloud)
        pts.counts[side].fill_(m)  # (from the shape: no host read)

    def update(self, gt_frame, pd_frame):
        """gt_frame, pd_frame: dicts with the reference's keys — "pano" and "intensities" [H, W] on both sides (world scale;
        depth 0 = dropped, the ground truth's -1 already 0 as extract_dataset_frame leaves it), "pano_mask" [H, W] (bool) on
        the ground-truth side with nerf_mvl, and optionally "local_points" [M, 3]: a side that brings its cloud is compared
        by it, a side that does not by the back-projection of its pano (which is what predict_frame_with_raydrop's
        local_points are, bit for bit).  Values are GPU tensors, or NumPy arrays that are moved once.  Returns nothing."""
        H, W = self.H, self.W
        gt_pano, pd_pano = _image(gt_frame["pano"], H, W, "gt pano"), _image(pd_frame["pano"], H, W, "pd pano")
        gt_int = _image(gt_frame["intensities"], H, W, "gt intensities")
        pd_int = _image(pd_frame["intensities"], H, W, "pd intensities")
        if self.state is None:
            self._alloc(gt_pano.device)
        mask = None
        if self.nerf_mvl:
            if "pano_mask" not in gt_frame:
                raise KeyError("NVSFrameEvaluator.update: a NeRF-MVL ground-truth frame needs 'pano_mask'")
            m = gt_frame["pano_mask"]
            if isinstance(m, np.ndarray):
                m = torch.from_numpy(np.ascontiguousarray(m != 0)).cuda(gt_pano.device)
            if not torch.is_tensor(m) or not m.is_cuda or m.numel() != H * W:
                raise ValueError(f"NVSFrameEvaluator.update: pano_mask must be [{H}, {W}] on the GPU or a NumPy array")
            self._mask.copy_((m if m.dtype in (torch.bool, torch.uint8) else m != 0).reshape(H, W))
            mask = self._mask.data_ptr()
        # point metrics: the full, uncropped clouds (run.py:219-221 passes them for NeRF-MVL too)
        pts = self.points
        gt_cloud, pd_cloud = gt_frame.get("local_points"), pd_frame.get("local_points")
        pts.state[0].fill_(0.0)
        if gt_cloud is None or pd_cloud is None:
            if not self._projects or self.intrinsics is None:
                raise ValueError("NVSFrameEvaluator.update: a frame without 'local_points' is back-projected from its pano: "
                                 "that needs intrinsics and the default points_capacity")
            self._gt3[..., 2].copy_(gt_pano)
            pts._project(pd_pano, self._gt3)
        if gt_cloud is not None:
            self._set_cloud(1, gt_cloud, "gt local_points")
        if pd_cloud is not None:
            self._set_cloud(0, pd_cloud, "pd local_points")
        pts._search()
        ws, ws_bytes = self._ws.data_ptr(), self._ws.numel() * 8
        _hip.call("lnh_nvs_eval_frame", gt_pano.data_ptr(), pd_pano.data_ptr(), gt_int.data_ptr(), pd_int.data_ptr(), mask, H, W,
                  self.intensity_scale, ws, ws_bytes)
        _hip.call("lnh_nvs_eval_ssim", gt_pano.data_ptr(), pd_pano.data_ptr(), mask, H, W, ws, ws_bytes)
        _hip.call("lnh_nvs_eval_finalize", H, W, ws, ws_bytes, pts.state[1].data_ptr(), self.state.data_ptr(),
                  self.state[1:].data_ptr() if self.max_frames else None, self.max_frames)

    def rows(self):
        """One device-to-host copy: (accumulator row, history rows of the frames kept), fp64, slots _hip.NVS_SLOT_NAMES."""
        if self.state is None:
            raise RuntimeError("NVSFrameEvaluator.rows: no frame has been evaluated")
        host = self.state.cpu().numpy()
        n = int(host[0][_SLOT["frames"]])
        return host[0], host[1:1 + min(n, self.max_frames)]

    def measure(self):
        """The means over the frames under the reference's eight keys (Python floats).  Refuses (RuntimeError) an evaluation
        with a frame the means cannot use, naming how many and, where the history holds one, which and why."""
        if self.state is None:
            raise RuntimeError("NVSFrameEvaluator.measure: no frame has been evaluated")
        acc, rows = self.rows()
        n = int(acc[_SLOT["frames"]])
        if n == 0:
            raise RuntimeError("NVSFrameEvaluator.measure: no frame has been evaluated")
        n_bad = int(acc[_SLOT["bad"]])
        if n_bad:
            bad = np.nonzero(rows[:, _SLOT["bad"]])[0]
            where = f"a frame beyond the {self.max_frames} kept in the history"
            if bad.size:
                k = int(bad[0])
                r = {name: rows[k, i] for name, i in _SLOT.items()}
                cnt, h, w = int(r["n"]), int(r["crop_h"]), int(r["crop_w"])
                if cnt == 0:
                    why = "its mask is empty"
                elif cnt != h * w:
                    why = f"its {cnt} masked pixels do not fill their {h} x {w} bounding rectangle"
                elif cnt < 7:
                    why = f"its {cnt} pixels are fewer than the SSIM window of 7"
                else:
                    why = ", ".join(f"{name} = {r[name]}" for name in METRICS if not np.isfinite(r[name])) or \
                        "its point clouds have no chamfer distance (an empty cloud)"
                where = f"frame {k}: {why}"
            raise RuntimeError(f"NVSFrameEvaluator.measure: {n_bad} of {n} frames cannot be averaged; {where}")
        return {name: float(acc[_SLOT[name]] / n) for name in METRICS}

    def report(self):
        """The lines run.py:242-244 prints."""
        m = self.measure()
        text = "Mean metrics:\n" + "\n".join(f"- {key}: {m[key]:.4f}" for key in sorted(m))
        print(text)
        return text


def eval_points_and_pano(gt_local_points, pd_local_points, gt_intensities, pd_intensities, gt_pano, pd_pano):
    """lidarnvs/eval.py:9-135 with its argument checks and messages: NumPy arrays in, a dict of Python floats out, computed on
    the device by a one-frame NVSFrameEvaluator with both clouds as given.  The inputs are not modified."""
    if not gt_local_points.ndim == 2 or not gt_local_points.shape[1] == 3:
        raise ValueError(f"gt_local_points must be (N, 3), but got {gt_local_points.shape}")
    if not pd_local_points.ndim == 2 or not pd_local_points.shape[1] == 3:
        raise ValueError(f"pd_local_points must be (M, 3), but got {pd_local_points.shape}")
    if not gt_intensities.ndim == 2:
        raise ValueError(f"gt_intensities must be (H, W), but got {gt_intensities.shape}")
    lidar_H, lidar_W = gt_intensities.shape
    if not pd_intensities.shape == (lidar_H, lidar_W):
        raise ValueError(f"pd_intensities must be (H, W), but got {pd_intensities.shape}")
    if not gt_pano.shape == (lidar_H, lidar_W):
        raise ValueError(f"gt_pano must be (H, W), but got {gt_pano.shape}")
    if not pd_pano.shape == (lidar_H, lidar_W):
        raise ValueError(f"pd_pano must be (H, W), but got {pd_pano.shape}")
    arrays = [gt_local_points, pd_local_points, gt_intensities, pd_intensities, gt_pano, pd_pano]
    if not all(isinstance(e, np.ndarray) for e in arrays):
        raise ValueError("All inputs must be numpy array.")
    if not torch.cuda.is_available():
        raise RuntimeError("eval_points_and_pano: needs a GPU (no CPU fallback)")
    cap = max(gt_local_points.shape[0], pd_local_points.shape[0], 1)
    ev = NVSFrameEvaluator(lidar_H, lidar_W, None, max_frames=1, points_capacity=cap)
    ev.update({"pano": gt_pano, "intensities": gt_intensities, "local_points": gt_local_points},
              {"pano": pd_pano, "intensities": pd_intensities, "local_points": pd_local_points})
    return ev.measure()


def evaluate_nvs(nvs, frames, raydrop=True, nerf_mvl=False, **predict_kwargs):
    """The loop of run.py:186-244: for every ground-truth frame dict (the keys of the reference's extract_dataset_frame: pano,
    intensities, lidar_K, lidar_pose, lidar_H, lidar_W, pano_mask with nerf_mvl) the prediction of `nvs` — a MeshNVS, a
    PointCloudNVS or a FieldNVS — by predict_frame_with_raydrop, or by predict_frame with raydrop=False, goes into one
    NVSFrameEvaluator.  Returns (mean metrics, the evaluator); the one host copy of the evaluation is measure()'s.  With
    raydrop=True only the two images of a prediction are used: its local_points are the back-projection of its pano, bit for
    bit, which the point metrics make themselves.  A model that offers predict_images_with_raydrop (MeshNVS, PointCloudNVS) is
    asked for the images alone, so no cloud is compacted and nothing reads the host per frame; FieldNVS returns images only.
    With raydrop=False the prediction's own local_points are compared (a mesh's hit points are not a back-projection), and
    their compaction in predict_frame is one host read per frame."""
    ev = None
    for gt in frames:
        H, W = int(gt["lidar_H"]), int(gt["lidar_W"])
        if raydrop:
            predict = getattr(nvs, "predict_images_with_raydrop", None) or nvs.predict_frame_with_raydrop
        else:
            predict = nvs.predict_frame
        pd = predict(lidar_K=gt["lidar_K"], lidar_pose=gt["lidar_pose"], lidar_H=H, lidar_W=W, **predict_kwargs)
        if ev is None:
            ev = NVSFrameEvaluator(H, W, gt["lidar_K"], nerf_mvl=nerf_mvl)
        elif (ev.H, ev.W) != (H, W):
            raise ValueError(f"evaluate_nvs: frames of one size wanted ({ev.H} x {ev.W}, then {H} x {W})")
        if raydrop:
            pd = {"pano": pd["pano"], "intensities": pd["intensities"]}
        ev.update({k: gt[k] for k in ("pano", "intensities", "pano_mask") if k in gt}, pd)
    if ev is None:
        raise ValueError("evaluate_nvs: no frames")
    return ev.measure(), ev


class FieldNVS:
    """The trained field behind the baselines' interface, so that evaluate_nvs scores it with the same meter.  trainer: a
    nerf.train_step.LidarTrainer; scale: the scene scale its depths are divided by; ema: render on the averaged weights when
    the trainer keeps them.  predict_frame_with_raydrop makes the frame's rays as test_step's callers do
    (lnh_lidar_frame_rays), calls trainer.test_step in eval mode and returns its images: {"pano": pred_depth / scale,
    "intensities": pred_intensity}, [H, W] on the device."""

    def __init__(self, trainer, scale, ema=True):
        self.trainer, self.scale, self.ema = trainer, float(scale), bool(ema)
        if not self.scale > 0:
            raise ValueError("FieldNVS: scale must be positive")

    def rays(self, lidar_K, lidar_pose, lidar_H, lidar_W):
        """test_step's `data` for one frame: rays_o_lidar / rays_d_lidar [1, H*W, 3], H_lidar, W_lidar."""
        _hip.require_symbols(("lnh_lidar_frame_rays",), "frame rays")
        K = [float(x) for x in (lidar_K.tolist() if hasattr(lidar_K, "tolist") else lidar_K)]
        H, W = int(lidar_H), int(lidar_W)
        pose = lidar_pose if torch.is_tensor(lidar_pose) else torch.from_numpy(np.asarray(lidar_pose, np.float32))
        if len(K) != 2 or H < 1 or W < 1 or tuple(pose.shape) != (4, 4):
            raise ValueError("FieldNVS: lidar_K must be (fov_up, fov), lidar_pose [4, 4], and the frame must not be empty")
        device = next(self.trainer.model.parameters()).device
        pose = pose.detach().to(device, torch.float32).contiguous()
        with torch.cuda.device(device):
            rays_o = torch.empty((1, H * W, 3), dtype=torch.float32, device=device)
            rays_d = torch.empty_like(rays_o)
            _hip.call("lnh_lidar_frame_rays", pose.data_ptr(), 1, 0, H, W, K[0], K[1], rays_o.data_ptr(), rays_d.data_ptr())
        return {"rays_o_lidar": rays_o, "rays_d_lidar": rays_d, "H_lidar": H, "W_lidar": W}

    def predict_frame_with_raydrop(self, lidar_K, lidar_pose, lidar_H, lidar_W):
        tr = self.trainer
        data = self.rays(lidar_K, lidar_pose, lidar_H, lidar_W)
        was_training = tr.model.training
        tr.model.eval()
        try:
            with (tr.ema_weights() if self.ema and tr.ema is not None else contextlib.nullcontext()):
                _, pred_intensity, pred_depth = tr.test_step(data)
        finally:
            tr.model.train(was_training)
        return {"pano": pred_depth[0] / self.scale, "intensities": pred_intensity[0]}
