"""TEST INFRASTRUCTURE — NumPy restatement of one row of the fused points meter (csrc/eval_points.hip, LNH_PTS_* of
include/lidarnerf_hip.h): what the reference's PointsMeter (nerf/utils.py:375-427) computes for a frame, with the per-frame
means taken in float64.  Built from the pieces the existing tests already pin: oracle.convert_ref's back-projection,
oracle.c_oracle's brute-force nearest neighbour (the float32 arithmetic of extern/chamfer3D) and oracle.metrics_ref.fscore."""
import numpy as np

from oracle import c_oracle, convert_ref, metrics_ref

SLOTS = ("chamfer", "fscore", "precision", "recall", "mean_pred", "mean_gt", "count_pred", "count_gt", "frames", "bad")


def metric_depths(pred_depth, gt, scale, nerf_mvl=False):
    """The two [H, W] float32 depth images in metres PointsMeter.update back-projects (evaluate.py:122-126, metrics.py:156)."""
    gt = np.asarray(gt, np.float32)
    gr = gt[..., 0]
    if nerf_mvl:
        gr = gr * np.where(gr == -1, 0, 1).astype(np.float32)
    s = np.float32(scale)
    return np.asarray(pred_depth, np.float32).reshape(gt.shape[:2]) / s, (gt[..., 2] * gr) / s


def clouds(pred_depth, gt, scale, K, nerf_mvl=False):
    P, G = metric_depths(pred_depth, gt, scale, nerf_mvl)
    zeros = np.zeros_like(P)
    return (convert_ref.pano_to_lidar_with_intensities(P, zeros, K)[:, :3].astype(np.float32),
            convert_ref.pano_to_lidar_with_intensities(G, zeros, K)[:, :3].astype(np.float32))


def row_of_clouds(a, b, threshold=0.05):
    """The row for two clouds [n, 3], [m, 3] float32 (both non-empty)."""
    d1, _ = c_oracle.chamfer_nn(a, b)
    d2, _ = c_oracle.chamfer_nn(b, a)
    m1, m2 = d1.astype(np.float64).mean(), d2.astype(np.float64).mean()
    p, r = float((d1 < np.float32(threshold)).mean()), float((d2 < np.float32(threshold)).mean())
    return dict(zip(SLOTS, (m1 + m2, metrics_ref.fscore(d1, d2, np.float32(threshold)), p, r, m1, m2, float(len(a)),
                            float(len(b)), 1.0, 0.0)))


def frame_row(pred_depth, gt, scale, K, threshold=0.05, nerf_mvl=False):
    return row_of_clouds(*clouds(pred_depth, gt, scale, K, nerf_mvl), threshold=threshold)
