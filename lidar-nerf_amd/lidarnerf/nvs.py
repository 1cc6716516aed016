"""Novel-view synthesis of a LiDAR frame from a triangle mesh on the device: LidarNVSMeshing.predict_frame and
predict_frame_with_raydrop of lidarnvs/lidarnvs_meshing.py:100-291 — ray casting (raycast.RaycastingScene), the
k-nearest-neighbour intensity lookup (knn.PointCloudIndex) and the range-image projection (convert), with every array kept on
the GPU.

What is not pinned against the reference: Open3D's order among equidistant neighbours and NumPy's float32 np.mean
(here: smallest index first, an fp64 rank-order sum rounded once), and its float64 pose matrices (here fp32).  The pose is taken
as affine (last row 0 0 0 1), which is what homo_project's division by w amounts to for a LiDAR pose.  The ray-drop U-Net of the
mesh baselines is lidarnerf/unet.py (RayDropUNet, inference), its training lidarnerf/unet_trainer.py.
MeshNVS.fit builds the mesh from a training sequence by TSDF fusion of its range images (lidarnerf/tsdf.py) — this
package's meshing function, not the reference's Poisson recipe — and MeshNVS.raydrop_dataset makes what the U-Net trainer takes.
No CPU fallback.

PointCloudNVS is the point-cloud baseline, LidarNVSPCGen of lidarnvs/lidarnvs_pcgen.py:16-248: the training cloud itself is
projected ("cp": closest point, "fpa": first-peak averaging over a z-buffer), turned back into a cloud, and masked by the
ray-drop MLP (lidarnerf/raydrop.py) — DESIGN §17."""
import math

import numpy as np
import torch

from . import convert
from .knn import PointCloudIndex, _check_k, _cloud
from .raycast import RaycastingScene
from .raydrop import IN_FEATURES
from .nvs_eval import FieldNVS, NVSFrameEvaluator, eval_points_and_pano, evaluate_nvs  # noqa: F401 (the evaluation)

CLOUD_KEYS = ("points", "point_intensities", "local_points", "local_point_intensities")


def _pose(lidar_pose, device):
    pose = lidar_pose if torch.is_tensor(lidar_pose) else torch.from_numpy(np.asarray(lidar_pose, np.float32))
    if tuple(pose.shape) != (4, 4):
        raise ValueError(f"MeshNVS: lidar_pose must be [4, 4], got {tuple(pose.shape)}")
    return pose.detach().to(device, torch.float32)


def _image(image, H, W, device, what):
    t = torch.from_numpy(np.array(image, dtype=np.float32)) if isinstance(image, np.ndarray) else image  # (a copy)
    if not torch.is_tensor(t) or t.numel() != H * W:
        raise ValueError(f"MeshNVS: {what} must hold {H} x {W} values")
    return t.detach().to(device, torch.float32).reshape(H, W)


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
    grid_resolution: of the cloud's PointCloudIndex.  set_raydrop(model) stores the model predict_frame_with_raydrop uses when it
    is given none (LidarNVSMeshing's ckpt_path: unet.RayDropUNet.from_checkpoint(path), or any callable)."""

    raydrop = None

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

    @classmethod
    def fit(cls, frames, *, resolution=256, voxel_size=None, truncation=None, box=None, margin=None, min_count=1, max_depth=None,
            intensity_interpolate_k=5, grid_resolution=None):
        """LidarNVSMeshing.fit with TSDF fusion as the meshing function: a fitted MeshNVS.  frames: an iterable of dicts with the
        keys of the reference's extract_dataset_frame that matter — pano [H,W], intensities [H,W], lidar_pose [4,4] (lidar ->
        world), lidar_K (fov_up, fov), lidar_H, lidar_W (tensors or NumPy arrays).  The world cloud and its intensities (the k-NN
        index) come from convert.pano_to_lidar_with_intensities and transform_points, of the pixels with a depth > 0; the same
        panos and poses go into a tsdf.TSDFVolume over `box` (min[3], max[3]; default: the cloud's bounds plus `margin`, whose
        default is 4 voxel_size, or 5 % of the largest extent without a voxel_size).  Frames of different H x W or K are
        integrated call by call, in the order given.  max_depth: None = 80, convert's default.  The fitted volume is kept as
        .volume."""
        from .tsdf import TSDFVolume
        frames = list(frames)
        if not frames:
            raise ValueError("MeshNVS.fit: no frames")
        if not torch.cuda.is_available():
            raise RuntimeError("MeshNVS.fit: needs a GPU (no CPU fallback)")
        dev = next((f["pano"].device for f in frames if torch.is_tensor(f["pano"]) and f["pano"].is_cuda),
                   torch.device("cuda", torch.cuda.current_device()))
        max_depth = 80 if max_depth is None else max_depth
        groups, clouds, intens = [], [], []
        with torch.cuda.device(dev):
            for f in frames:
                H, W = int(f["lidar_H"]), int(f["lidar_W"])
                K = tuple(float(x) for x in (f["lidar_K"].tolist() if hasattr(f["lidar_K"], "tolist") else f["lidar_K"]))
                pano, inten = _image(f["pano"], H, W, dev, "pano"), _image(f["intensities"], H, W, dev, "intensities")
                pose = _pose(f["lidar_pose"], dev)
                seen = torch.isfinite(pano) & (pano > 0)  # (NeRF-MVL marks pixels outside its window with -1)
                local4 = convert.pano_to_lidar_with_intensities(torch.where(seen, pano, torch.zeros_like(pano)), inten, K)
                clouds.append(transform_points(local4[:, :3].contiguous(), pose))
                intens.append(local4[:, 3].contiguous())
                if not groups or groups[-1][0] != (H, W, K):
                    groups.append(((H, W, K), [], []))
                groups[-1][1].append(pano)
                groups[-1][2].append(pose)
            points, point_intensities = torch.cat(clouds), torch.cat(intens)
            if points.shape[0] == 0:
                raise ValueError("MeshNVS.fit: the frames hold no pixel with a depth")
            if box is None:
                lo, hi = points.min(0).values.double().cpu().numpy(), points.max(0).values.double().cpu().numpy()
                if margin is None:
                    margin = 4.0 * float(voxel_size) if voxel_size is not None else 0.05 * float((hi - lo).max())
                box = (lo - float(margin), hi + float(margin))
            volume = TSDFVolume(box, resolution=resolution, voxel_size=voxel_size, truncation=truncation, device=dev)
            for (_, _, K), panos, poses in groups:
                volume.integrate(torch.stack(panos), torch.stack(poses), K, max_depth=max_depth)
            fitted = cls(volume.scene(min_count=min_count), points, point_intensities,
                         intensity_interpolate_k=intensity_interpolate_k, grid_resolution=grid_resolution)
        fitted.volume = volume
        return fitted

    def raydrop_dataset(self, frames):
        """The reference's generate_raydrop_data_meshing and RaydropDataset.collate_fn in one: (images f32 [N,10,H,W], masks f32
        [N,H,W]) on the device for frames of one size — raydrop_features of every frame's pose, one after another, and
        pano != 0 as floats.  What unet_trainer.RayDropUNetTrainer.train_step / train_epoch take."""
        frames = list(frames)
        if not frames:
            raise ValueError("MeshNVS.raydrop_dataset: no frames")
        H, W = int(frames[0]["lidar_H"]), int(frames[0]["lidar_W"])
        images, masks = [], []
        for f in frames:
            if (int(f["lidar_H"]), int(f["lidar_W"])) != (H, W):
                raise ValueError(f"MeshNVS.raydrop_dataset: frames of {int(f['lidar_H'])} x {int(f['lidar_W'])} and {H} x {W} do not "
                                 "stack")
            images.append(self.raydrop_features(f["lidar_K"], f["lidar_pose"], H, W))
            masks.append((_image(f["pano"], H, W, self.device, "pano") != 0).to(torch.float32))
        return torch.cat(images, dim=0).contiguous(), torch.stack(masks)

    def set_raydrop(self, model):
        """Store the ray-drop model (a unet.RayDropUNet, or any callable from the [1,10,H,W] feature image to [1,1,H,W] logits) that
        predict_frame_with_raydrop and predict_images_with_raydrop use when none is passed; None removes it.  Returns self."""
        if model is not None and not callable(model):
            raise TypeError("MeshNVS.set_raydrop: the model must be callable")
        self.raydrop = model
        return self

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
    def predict_images_with_raydrop(self, lidar_K, lidar_pose, lidar_H, lidar_W, model=None):
        """The images of predict_frame_with_raydrop without its clouds: pano, intensities (both multiplied by the mask) and
        hit_dict.  Nothing reads the host (the clouds' length is the one host read of predict_frame_with_raydrop), so with a
        unet.RayDropUNet the whole call can be captured."""
        if model is None:
            model = self.raydrop
        if model is None:
            raise TypeError("MeshNVS.predict_frame_with_raydrop() missing 1 required positional argument: 'model' "
                            "(pass one, or store one with set_raydrop)")
        H, W = int(lidar_H), int(lidar_W)
        pose = _pose(lidar_pose, self.device)
        frame = self.predict_frame(lidar_K, pose, H, W, compact=False)
        images = self.scene.raydrop_features(lidar_K, pose, H, W, intensities=frame["intensities"])
        logits = model(images)
        if not torch.is_tensor(logits) or logits.numel() != H * W:
            raise ValueError(f"MeshNVS.predict_frame_with_raydrop: the model must return [1, 1, {H}, {W}] logits")
        keep = (torch.sigmoid(logits.detach().to(self.device, torch.float32)) > 0.5).to(torch.float32).reshape(H, W)
        return {"pano": frame["pano"] * keep, "intensities": frame["intensities"] * keep, "hit_dict": frame["hit_dict"]}

    @torch.no_grad()
    def predict_frame_with_raydrop(self, lidar_K, lidar_pose, lidar_H, lidar_W, model=None):
        """lidarnvs_meshing.py:170-291.  model: any callable from the [1,10,H,W] feature image to [1,1,H,W] logits (a
        unet.RayDropUNet is the reference's network); None: the model stored with set_raydrop.  A pixel is kept where
        sigmoid(logit) > 0.5.  pano and intensities are multiplied by that mask and turned back into the clouds
        (convert.pano_to_lidar_with_intensities, then the pose)."""
        pose = _pose(lidar_pose, self.device)
        out = self.predict_images_with_raydrop(lidar_K, pose, lidar_H, lidar_W, model)
        local4 = convert.pano_to_lidar_with_intensities(out["pano"], out["intensities"], lidar_K)
        local_points = local4[:, :3].contiguous()
        local_inten = local4[:, 3].contiguous()
        return {"pano": out["pano"], "intensities": out["intensities"], "points": transform_points(local_points, pose),
                "point_intensities": local_inten, "local_points": local_points, "local_point_intensities": local_inten,
                "hit_dict": out["hit_dict"]}

    def evaluate(self, frames, raydrop=True, nerf_mvl=False, **predict_kwargs):
        """nvs_eval.evaluate_nvs on this model: (mean metrics under the reference's eight keys, the evaluator)."""
        return evaluate_nvs(self, frames, raydrop=raydrop, nerf_mvl=nerf_mvl, **predict_kwargs)


PCGEN_KEYS = ("pano", "intensities") + CLOUD_KEYS


class PointCloudNVS:
    """LidarNVSPCGen with every array on the device.  points float [N,3] / point_intensities float [N]: the world-frame
    training cloud (tensors or NumPy arrays; `device` or the current GPU), or None until fit().  raycasting: "cp"
    (convert.lidar_to_pano_with_intensities) or "fpa" (..._fpa with z_buffer_len).  raydrop: a raydrop.RayDropMLP or any callable
    from the [H*W, 5] rows (direction, depth, intensity) to [H*W, 1]; a ray is kept where the output is > 0.5."""

    def __init__(self, points=None, point_intensities=None, raycasting="cp", raydrop=None, z_buffer_len=10, device=None):
        if raycasting not in ("cp", "fpa"):
            raise ValueError(f"PointCloudNVS: raycasting must be 'cp' or 'fpa', got {raycasting!r}")
        if int(z_buffer_len) < 1:
            raise ValueError("PointCloudNVS: z_buffer_len must be at least 1")
        if not torch.cuda.is_available():
            raise RuntimeError("PointCloudNVS: needs a GPU (no CPU fallback)")
        self.raycasting, self.raydrop, self.z_buffer_len = raycasting, raydrop, int(z_buffer_len)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.points = self.point_intensities = None
        if points is not None:
            self._set_cloud(points, point_intensities)

    def _set_cloud(self, points, point_intensities):
        def tensor(a):
            return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        pts, inten = tensor(points), tensor(point_intensities)
        if not torch.is_tensor(pts) or pts.dim() != 2 or pts.shape[1] != 3 or not pts.is_floating_point():
            raise ValueError("PointCloudNVS: points must be a float [N, 3] tensor or NumPy array")
        if not torch.is_tensor(inten) or not inten.is_floating_point() or inten.numel() != pts.shape[0]:
            raise ValueError(f"PointCloudNVS: point_intensities must be {pts.shape[0]} floats")
        self.points = pts.detach().to(self.device, torch.float32).contiguous()
        self.point_intensities = inten.detach().reshape(-1).to(self.device, torch.float32).contiguous()

    def fit(self, frames):
        """frames: an iterable of dicts with "points" [n,3] and "point_intensities" [n] in WORLD coordinates (what the
        reference's extract_dataset_frame returns); their concatenation becomes the cloud, which is all the reference's fit
        does."""
        frames = list(frames)
        if not frames:
            raise ValueError("PointCloudNVS.fit: no frames")

        def tensor(a):
            return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(self.device, torch.float32)
        self._set_cloud(torch.cat([tensor(f["points"]).reshape(-1, 3) for f in frames]),
                        torch.cat([tensor(f["point_intensities"]).reshape(-1) for f in frames]))
        return self

    def _cloud(self):
        if self.points is None:
            raise RuntimeError("PointCloudNVS: no cloud yet (pass points or call fit)")
        return self.points, self.point_intensities

    def directions(self, lidar_K, lidar_H, lidar_W):
        """get_direction of lidarnvs_pcgen.py:236-248 in fp32 on the device: [H, W, 3], the operations in the reference's order."""
        H, W = int(lidar_H), int(lidar_W)
        fov_up, fov = float(lidar_K[0]), float(lidar_K[1])
        i = torch.arange(W, dtype=torch.float32, device=self.device)[None, :].expand(H, W)
        j = torch.arange(H, dtype=torch.float32, device=self.device)[:, None].expand(H, W)
        beta = -(i - W / 2) / W * 2 * math.pi
        alpha = (fov_up - j / H * fov) / 180 * math.pi
        ca = torch.cos(alpha)
        return torch.stack([ca * torch.cos(beta), ca * torch.sin(beta), torch.sin(alpha)], -1)

    def predict_frame(self, lidar_K, lidar_pose, lidar_H, lidar_W, compact=True):
        """The reference's predict_dict as device tensors: pano f32 [H,W], intensities f32 [H,W] and, with compact=True, the
        clouds read back from them — local_points [M,3], local_point_intensities [M], points [M,3] (the pose applied),
        point_intensities [M].  With compact=False only the two images are returned and nothing reads the host."""
        H, W = int(lidar_H), int(lidar_W)
        pose = _pose(lidar_pose, self.device)
        points, inten = self._cloud()
        rows = torch.cat([world_to_lidar(points, pose), inten[:, None]], dim=1)
        if self.raycasting == "cp":
            pano, intensities = convert.lidar_to_pano_with_intensities(rows, H, W, lidar_K)
        else:
            pano, intensities = convert.lidar_to_pano_with_intensities_fpa(rows, H, W, lidar_K, z_buffer_len=self.z_buffer_len)
        out = {"pano": pano, "intensities": intensities}
        if compact:
            out.update(self._clouds(pano, intensities, lidar_K, pose))
        return out

    @staticmethod
    def _clouds(pano, intensities, lidar_K, pose):
        local4 = convert.pano_to_lidar_with_intensities(pano, intensities, lidar_K)
        local_points = local4[:, :3].contiguous()
        local_inten = local4[:, 3].contiguous()
        return {"points": transform_points(local_points, pose), "point_intensities": local_inten,
                "local_points": local_points, "local_point_intensities": local_inten}

    def raydrop_rows(self, lidar_K, lidar_pose, lidar_H, lidar_W, gt_pano=None, frame=None):
        """The ray-drop MLP's input rows of a frame, [H*W, 5]: direction, predicted depth, predicted intensity (the order of
        run_network's cat).  With gt_pano [H,W] the training rows [n, 6] after the filtering of raydrop_train_pcgen.py:317-328:
        only pixels with gt_pano > -1, target 0 where gt_pano == 0, else 1."""
        H, W = int(lidar_H), int(lidar_W)
        if frame is None:
            frame = self.predict_frame(lidar_K, lidar_pose, H, W, compact=False)
        rows = torch.cat([self.directions(lidar_K, H, W).reshape(-1, 3), frame["pano"].reshape(-1, 1),
                          frame["intensities"].reshape(-1, 1)], dim=1)
        if gt_pano is None:
            return rows
        gt = torch.from_numpy(np.ascontiguousarray(gt_pano)) if isinstance(gt_pano, np.ndarray) else gt_pano
        gt = gt.detach().to(self.device, torch.float32).reshape(-1)
        if gt.numel() != H * W:
            raise ValueError(f"PointCloudNVS.raydrop_rows: gt_pano must be [{H}, {W}]")
        target = torch.where(gt == 0, 0.0, 1.0).to(torch.float32)
        return torch.cat([rows, target[:, None]], dim=1)[gt > -1]

    @torch.no_grad()
    def predict_images_with_raydrop(self, lidar_K, lidar_pose, lidar_H, lidar_W, raydrop=None):
        """The images of predict_frame_with_raydrop without its clouds: pano and intensities multiplied by the mask `output >
        0.5` — unless the mask is zero everywhere, which leaves the frame as it is (the reference's rule).  Nothing reads the
        host (the clouds' length is the one host read of predict_frame_with_raydrop)."""
        model = self.raydrop if raydrop is None else raydrop
        if model is None:
            raise RuntimeError("PointCloudNVS.predict_frame_with_raydrop: no ray-drop model")
        H, W = int(lidar_H), int(lidar_W)
        pose = _pose(lidar_pose, self.device)
        frame = self.predict_frame(lidar_K, pose, H, W, compact=False)
        rows = self.raydrop_rows(lidar_K, pose, H, W, frame=frame)
        assert rows.shape == (H * W, IN_FEATURES)
        out = model(rows)
        if not torch.is_tensor(out) or tuple(out.shape) != (H * W, 1):
            raise ValueError(f"PointCloudNVS.predict_frame_with_raydrop: the model must return [{H * W}, 1] outputs")
        keep = (out.detach().to(self.device, torch.float32) > 0.5).reshape(H, W)
        keep = torch.where(keep.any(), keep, torch.ones_like(keep)).to(torch.float32)
        return {"pano": frame["pano"] * keep, "intensities": frame["intensities"] * keep}

    @torch.no_grad()
    def predict_frame_with_raydrop(self, lidar_K, lidar_pose, lidar_H, lidar_W, raydrop=None):
        """lidarnvs_pcgen.py:131-194: the masked images of predict_images_with_raydrop, turned back into the clouds."""
        pose = _pose(lidar_pose, self.device)
        result = self.predict_images_with_raydrop(lidar_K, pose, lidar_H, lidar_W, raydrop)
        result.update(self._clouds(result["pano"], result["intensities"], lidar_K, pose))
        return result

    def evaluate(self, frames, raydrop=True, nerf_mvl=False, **predict_kwargs):
        """nvs_eval.evaluate_nvs on this model: (mean metrics under the reference's eight keys, the evaluator)."""
        return evaluate_nvs(self, frames, raydrop=raydrop, nerf_mvl=nerf_mvl, **predict_kwargs)
