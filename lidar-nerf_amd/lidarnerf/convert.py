"""Point cloud <-> range image on the GPU — same function names and argument meaning as lidarnerf/convert.py
(lidar_to_pano_with_intensities_with_bbox_mask 4-97, lidar_to_pano_with_intensities 99-160, lidar_to_pano 163-191,
pano_to_lidar_with_intensities 194-237, pano_to_lidar 240-254, lidar_to_pano_with_intensities_fpa 253-361).  The reference
loops over points in Python; here one atomic-min pass + one resolve pass, and for the z-buffer ("fpa") variant a
count / scan / scatter / resolve pipeline (csrc/convert.hip).

Inputs may be NumPy arrays (results come back as NumPy, like the reference) or CUDA tensors (results stay on the GPU).
Values are float32 (the reference stores the same float32 values in float64 arrays; the fpa averages are formed in float64
and rounded to float32 once).
"""
import numpy as np
import torch

from . import _hip


def _to_gpu(a, cols=None):
    was_np = isinstance(a, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() if was_np else a
    if not t.is_cuda:
        raise RuntimeError("lidarnerf.convert: tensors must live on the GPU (no CPU fallback)")
    t = t.float().contiguous()
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError(f"expected an [N, {cols}] array, got {tuple(t.shape)}")
    return t, was_np


def lidar_to_pano_with_intensities(local_points_with_intensities, lidar_H, lidar_W, lidar_K, max_depth=80):
    pts, was_np = _to_gpu(local_points_with_intensities, 4)
    fov_up, fov = float(lidar_K[0]), float(lidar_K[1])
    H, W = int(lidar_H), int(lidar_W)
    keys = torch.empty(H * W, dtype=torch.int64, device=pts.device)
    pano = torch.empty((H, W), dtype=torch.float32, device=pts.device)
    inten = torch.empty((H, W), dtype=torch.float32, device=pts.device)
    _hip.call("lnh_lidar_to_pano", pts.data_ptr(), pts.shape[0], H, W, fov_up, fov, float(max_depth), keys.data_ptr(),
              pano.data_ptr(), inten.data_ptr())
    if was_np:
        return pano.cpu().numpy().astype(np.float64), inten.cpu().numpy().astype(np.float64)
    return pano, inten


def lidar_to_pano(local_points, lidar_H, lidar_W, lidar_K, max_depth=80):
    if isinstance(local_points, np.ndarray):
        p4 = np.concatenate([local_points, np.zeros((local_points.shape[0], 1), local_points.dtype)], axis=1)
    else:
        p4 = torch.cat([local_points, torch.zeros_like(local_points[:, :1])], dim=1)
    return lidar_to_pano_with_intensities(p4, lidar_H, lidar_W, lidar_K, max_depth)[0]


def pano_to_lidar_with_intensities(pano, intensities, lidar_K):
    p, was_np = _to_gpu(pano)
    it = None if intensities is None else _to_gpu(intensities)[0]
    H, W = p.shape
    fov_up, fov = float(lidar_K[0]), float(lidar_K[1])
    pts = torch.empty((H * W, 4), dtype=torch.float32, device=p.device)
    valid = torch.empty(H * W, dtype=torch.uint8, device=p.device)
    _hip.call("lnh_pano_to_lidar", p.data_ptr(), None if it is None else it.data_ptr(), H, W, fov_up, fov,
              pts.data_ptr(), valid.data_ptr())
    out = pts[valid.bool()]  # pixel (row-major) order, like np.where
    return out.cpu().numpy() if was_np else out


def pano_to_lidar(pano, lidar_K):
    return pano_to_lidar_with_intensities(pano, None, lidar_K)[:, :3]


FPA_THRESHOLD = 0.2  # parse_z_buffer's default (convert.py:331); the reference never passes another value


def lidar_to_pano_with_intensities_fpa(local_points_with_intensities, lidar_H, lidar_W, lidar_K, max_depth=80,
                                       z_buffer_len=10):
    """First-peak averaging over a per-pixel z-buffer (include/lidarnerf_hip.h, lnh_lidar_to_pano_fpa).  The result depends
    on the order of the points, as the reference's does."""
    _hip.require_symbols(("lnh_lidar_to_pano_fpa", "lnh_lidar_to_pano_fpa_workspace_size"), "fpa conversion")
    pts, was_np = _to_gpu(local_points_with_intensities, 4)
    fov_up, fov = float(lidar_K[0]), float(lidar_K[1])
    H, W, N = int(lidar_H), int(lidar_W), pts.shape[0]
    if H < 1 or W < 1 or int(z_buffer_len) < 1:
        raise ValueError(f"lidar_to_pano_with_intensities_fpa: bad size H={H} W={W} z_buffer_len={z_buffer_len}")
    need = int(_hip.lib().lnh_lidar_to_pano_fpa_workspace_size(N, H, W))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=pts.device)  # (an unsupported shape: the call says why)
    pano = torch.empty((H, W), dtype=torch.float32, device=pts.device)
    inten = torch.empty((H, W), dtype=torch.float32, device=pts.device)
    _hip.call("lnh_lidar_to_pano_fpa", pts.data_ptr(), N, H, W, fov_up, fov, float(max_depth), int(z_buffer_len),
              FPA_THRESHOLD, ws.data_ptr(), ws.numel(), pano.data_ptr(), inten.data_ptr())
    if was_np:
        return pano.cpu().numpy().astype(np.float64), inten.cpu().numpy().astype(np.float64)
    return pano, inten


def _bbox_window(bbox_local, lidar_H, lidar_W, lidar_K):
    """Rows r_min:r_max and columns c_min:c_max of the projected box corners, as convert.py:46-66 computes them on the host."""
    if isinstance(bbox_local, torch.Tensor):
        bbox_local = bbox_local.detach().cpu().numpy()  # (8 corners; the point cloud itself never leaves the device)
    bbox_local = np.asarray(bbox_local)
    if bbox_local.ndim != 2 or bbox_local.shape[1] != 4:
        raise ValueError(f"expected an [8, 4] array of box corners, got {bbox_local.shape}")
    fov_up, fov = lidar_K
    fov_down = fov - fov_up
    r_min, r_max, c_min, c_max = 1e5, -1, 1e5, -1
    for bbox_local_point in bbox_local:
        x, y, z, _ = bbox_local_point
        beta = np.pi - np.arctan2(y, x)
        alpha = np.arctan2(z, np.sqrt(x**2 + y**2)) + fov_down / 180 * np.pi
        c = int(round(beta / (2 * np.pi / lidar_W)))
        r = int(round(lidar_H - alpha / (fov / 180 * np.pi / lidar_H)))
        if r >= lidar_H or r < 0 or c >= lidar_W or c < 0:
            continue
        r_min, r_max, c_min, c_max = min(r_min, r), max(r_max, r), min(c_min, c), max(c_max, c)
    if r_max < 0:
        raise ValueError("lidar_to_pano_with_intensities_with_bbox_mask: no corner of bbox_local lands in the image "
                         "(the reference fails on a float slice index here)")
    return r_min, r_max, c_min, c_max


def lidar_to_pano_with_intensities_with_bbox_mask(local_points_with_intensities, lidar_H, lidar_W, lidar_K, bbox_local,
                                                  max_depth=80, max_intensity=255.0):
    """Closest point per pixel inside the window of the projected box (pano = -1 outside it), intensity / max_intensity."""
    _hip.require_symbols(("lnh_lidar_to_pano_masked",), "bbox-mask conversion")
    pts, was_np = _to_gpu(local_points_with_intensities, 4)
    fov_up, fov = float(lidar_K[0]), float(lidar_K[1])
    H, W = int(lidar_H), int(lidar_W)
    r0, r1, c0, c1 = _bbox_window(bbox_local, H, W, lidar_K)
    keys = torch.empty(H * W, dtype=torch.int64, device=pts.device)
    pano = torch.empty((H, W), dtype=torch.float32, device=pts.device)
    inten = torch.empty((H, W), dtype=torch.float32, device=pts.device)
    _hip.call("lnh_lidar_to_pano_masked", pts.data_ptr(), pts.shape[0], H, W, fov_up, fov, float(max_depth), r0, r1, c0, c1,
              float(max_intensity), keys.data_ptr(), pano.data_ptr(), inten.data_ptr())
    if was_np:
        return pano.cpu().numpy().astype(np.float64), inten.cpu().numpy().astype(np.float64)
    return pano, inten
