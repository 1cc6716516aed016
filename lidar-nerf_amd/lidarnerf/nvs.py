"""Novel-view synthesis of a LiDAR frame from a triangle mesh on the device: LidarNVSMeshing.predict_frame and
predict_frame_with_raydrop of lidarnvs/lidarnvs_meshing.py:100-291 — ray casting (raycast.RaycastingScene), the
k-nearest-neighbour intensity lookup (knn.PointCloudIndex) and the range-image projection (convert), with every array kept on
the GPU.

What is not pinned against the reference: Open3D's order among equidistant neighbours and NumPy's float32 np.mean
(here: smallest index first, an fp64 rank-order sum rounded once), and its float64 pose matrices (here fp32).  The pose is taken
as affine (last row 0 0 0 1), which is what homo_project's division by w amounts to for a LiDAR pose.  The ray-drop U-Net, its
training and the meshing itself (fit) are not part of this.  No CPU fallback."""
import math

import numpy as np
import torch

from . import convert
from .knn import PointCloudIndex, _check_k, _cloud
from .raycast import RaycastingScene

CLOUD_KEYS = ("points", "point_intensities", "local_points", "local_point_intensities")


def _pose(lidar_pose, device):
    pose = lidar_pose if torch.is_tensor(lidar_pose) else torch.from_numpy(np.asarray(lidar_pose, np.float32))
    if tuple(pose.shape) != (4, 4):
        raise ValueError(f"MeshNVS: lidar_pose must be [4, 4], got {tuple(pose.shape)}")
    return pose.detach().to(device, torch.float32)


def transform_points(points, pose):
    """pose [4,4] (affine) applied to points [N,3] in fp32, one rounded operation per operator:
    ((x * A[:,0] + y * A[:,1]) + z * A[:,2]) + t.  GPU tensors."""
    A, t = pose[:3, :3], pose[:3, 3]
    return ((points[:, 0:1] * A[:, 0] + points[:, 1:2] * A[:, 1]) + points[:, 2:3] * A[:, 2]) + t


def inverse_pose(pose):
    """The inverse of an affine pose [4,4] on the device in fp32, by cofactors (no host read, no solver): rows of A^-1 are the
    cross products of A's columns over the determinant, the translation is -(A^-1 t)."""
    A, t = pose[:3, :3], pose[:3, 3]
    c0 = torch.linalg.cross(A[:, 1], A[:, 2])
    c1 = torch.linalg.cross(A[:, 2], A[:, 0])
    c2 = torch.linalg.cross(A[:, 0], A[:, 1])
    det = (A[:, 0] * c0).sum()
    inv = torch.stack([c0, c1, c2]) / det
    back = -((inv[:, 0] * t[0] + inv[:, 1] * t[1]) + inv[:, 2] * t[2])
    return torch.cat([torch.cat([inv, back[:, None]], dim=1), pose[3:4]], dim=0)  # (the last row of an affine pose is its own)


def world_to_lidar(points, lidar_pose):
    """World -> lidar frame: ct.project.homo_project(points, pose_to_T(lidar_pose)) in fp32 on the device."""
    return transform_points(points, inverse_pose(lidar_pose))


class MeshNVS:
    """scene: a raycast.RaycastingScene (for instance LidarTrainer.mesh_scene()).  points float [N,3] / point_intensities
    float [N]: the world-frame training cloud LidarNVSMeshing.fit keeps (tensors or NumPy arrays; moved to the scene's GPU).
    intensity_interpolate_k: neighbours averaged per hit point (lidarnvs_poisson.py's default 5; run.py passes 9).
    grid_resolution: of the cloud's PointCloudIndex."""

    def __init__(self, scene, points, point_intensities, intensity_interpolate_k=5, grid_resolution=None):
        if not isinstance(scene, RaycastingScene):
            raise TypeError("MeshNVS: scene must be a lidarnerf.raycast.RaycastingScene")
        self.k = _check_k(intensity_interpolate_k)
        inten = torch.from_numpy(np.ascontiguousarray(point_intensities)) if isinstance(point_intensities, np.ndarray) \
            else point_intensities
        if not torch.is_tensor(inten) or not inten.is_floating_point():
            raise ValueError("MeshNVS: point_intensities must be a float tensor or NumPy array")
        points = _cloud(points)
        if inten.numel() != points.shape[0]:
            raise ValueError(f"MeshNVS: {inten.numel()} intensities for {points.shape[0]} points")
        self.scene = scene
        self.device = scene.device
        if points.is_cuda and points.device != self.device:
            raise RuntimeError(f"MeshNVS: points on {points.device}, the scene on {self.device}")
        self.index = PointCloudIndex(points.to(self.device), grid_resolution=grid_resolution)
        self.points = self.index.points
        self.point_intensities = inten.detach().reshape(-1).to(self.device, torch.float32).contiguous()

    def predict_frame(self, lidar_K, lidar_pose, lidar_H, lidar_W, compact=True):
        """The reference's predict_dict as device tensors: pano f32 [H,W], intensities f32 [H,W], hit_dict (intersect_lidar's,
        unfiltered) and, with compact=True, the clouds of the hit points — points [M,3], point_intensities [M], local_points
        [M,3], local_point_intensities [M] — through one boolean index at the end (the only host read; with compact=False
        there is none and the call can be captured)."""
        H, W = int(lidar_H), int(lidar_W)
        pose = _pose(lidar_pose, self.device)
        hit = self.scene.intersect_lidar(lidar_K, pose, H, W)
        masks = hit["masks"]
        local = world_to_lidar(hit["points"], pose)
        inten = self.index.mean_of_neighbours(hit["points"], self.point_intensities, self.k, valid=masks)
        # the [H*W, 4] array is NOT compacted: a ray that missed becomes a NaN row, which the projection skips like any point
        # it cannot place, and the index tie rule of the closest-point pass sees the order of the compacted cloud
        rows = torch.cat([local, inten[:, None]], dim=1)
        rows = torch.where(masks[:, None], rows, torch.full_like(rows, math.nan))
        pano, intensities = convert.lidar_to_pano_with_intensities(rows, H, W, lidar_K)
        out = {"pano": pano, "intensities": intensities, "hit_dict": hit}
        if compact:
            out["points"] = hit["points"][masks]
            out["point_intensities"] = inten[masks]
            out["local_points"] = local[masks]
            out["local_point_intensities"] = out["point_intensities"]
        return out

    def raydrop_features(self, lidar_K, lidar_pose, lidar_H, lidar_W):
        """The [1, 10, H, W] image of RaycastingScene.raydrop_features with predict_frame's intensity image in channel 6."""
        pose = _pose(lidar_pose, self.device)
        frame = self.predict_frame(lidar_K, pose, lidar_H, lidar_W, compact=False)
        return self.scene.raydrop_features(lidar_K, pose, lidar_H, lidar_W, intensities=frame["intensities"])

    @torch.no_grad()
    def predict_frame_with_raydrop(self, lidar_K, lidar_pose, lidar_H, lidar_W, model):
        """lidarnvs_meshing.py:170-291.  model: any callable from the [1,10,H,W] feature image to [1,1,H,W] logits; a pixel
        is kept where sigmoid(logit) > 0.5.  pano and intensities are multiplied by that mask and turned back into the clouds
        (convert.pano_to_lidar_with_intensities, then the pose)."""
        H, W = int(lidar_H), int(lidar_W)
        pose = _pose(lidar_pose, self.device)
        frame = self.predict_frame(lidar_K, pose, H, W, compact=False)
        images = self.scene.raydrop_features(lidar_K, pose, H, W, intensities=frame["intensities"])
        logits = model(images)
        if not torch.is_tensor(logits) or logits.numel() != H * W:
            raise ValueError(f"MeshNVS.predict_frame_with_raydrop: the model must return [1, 1, {H}, {W}] logits")
        keep = (torch.sigmoid(logits.detach().to(self.device, torch.float32)) > 0.5).to(torch.float32).reshape(H, W)
        pano = frame["pano"] * keep
        intensities = frame["intensities"] * keep
        local4 = convert.pano_to_lidar_with_intensities(pano, intensities, lidar_K)
        local_points = local4[:, :3].contiguous()
        local_inten = local4[:, 3].contiguous()
        return {"pano": pano, "intensities": intensities, "points": transform_points(local_points, pose),
                "point_intensities": local_inten, "local_points": local_points, "local_point_intensities": local_inten,
                "hit_dict": frame["hit_dict"]}
