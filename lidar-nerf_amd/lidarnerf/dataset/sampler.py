"""Training batches drawn on the device from a preloaded sequence (csrc/lidar_sample.hip).

The reference builds a batch on the host side of every step: KITTI360Dataset.collate / NeRFMVLDataset.collate pick the
frame, get_lidar_rays draws patch corners with two randint calls, forms indices, angles and directions, rotates them by the
pose, and a gather fetches the targets (lidarnerf/dataset/base_dataset.py:16-105, kitti360_dataset.py:123-159) — two dozen
small launches per step in torch.  LidarBatchSampler does all of it in ONE launch (plus a one-thread launch that moves its
cursor on), reading the frame of the step and the position of its random stream from device memory: LidarTrainer.step_sampled
captures both launches at the head of the step's graph, and a training step then needs no host input at all.

What is kept from the reference, quirks included: the row count n = (min(N, H*W) // (px*py)) * px*py, corners over
[0, H-px) x [0, W-py) (the last row / column is never drawn), row-major pixels inside a patch (rays.patch_indices), one frame
per batch, frames shuffled per epoch.  What is not reproduced: torch's randint stream — the generator is Philox-4x32-10
(include/lidarnerf_hip.h, lnh_lidar_sample_batch), restated in tests/sampler_ref.py."""
import itertools

import numpy as np
import torch

from .. import _hip

_UIDS = itertools.count(1)


def patch_shape(patch_size):
    """(px, py) of a patch_size in the three forms get_lidar_rays takes: an int, [p] or [px, py]."""
    if isinstance(patch_size, (int, np.integer)):
        return int(patch_size), int(patch_size)
    ps = [int(v) for v in patch_size]
    if len(ps) == 1:
        return ps[0], ps[0]
    if len(ps) == 2:
        return ps[0], ps[1]
    raise ValueError(f"patch_size: an int, [p] or [px, py], not {patch_size!r}")


def batch_rows(num_rays, H, W, px, py):
    """Rays of one batch (base_dataset.py:45-52): whole patches out of min(num_rays, H*W)."""
    n = min(int(num_rays), H * W)
    return n // (px * py) * (px * py) if px > 0 else n


class LidarBatchSampler:
    """sequence: the dict dataset.range_image.load_sequence returns, preloaded on the GPU (poses_lidar [F,4,4] f32,
    images_lidar [F,H,W,3] f16 / f32, H_lidar, W_lidar); intrinsics (fov_up, fov) in degrees; patch_size as in
    get_lidar_rays; stream_id: the data-parallel rank (ranks draw different batches from one seed).

    The sampler owns the frame order `perm`, the cursor [step within the epoch, draws so far] and the output buffers, all on
    the device.  Until the first new_epoch() the frames come in file order."""

    def __init__(self, sequence, intrinsics, num_rays=4096, patch_size=1, seed=0, stream_id=0):
        poses, images = sequence["poses_lidar"], sequence["images_lidar"]
        if images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"LidarBatchSampler: images_lidar must be [F, H, W, 3] (ray-drop, intensity, depth), got "
                             f"{tuple(images.shape)}")
        for name, t in (("poses_lidar", poses), ("images_lidar", images)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f"lidarnerf_hip: LidarBatchSampler: sequence[{name!r}] must live on the GPU (no CPU path in "
                                   "this library; load_sequence(..., device=, preload=True))")
        H, W = int(sequence["H_lidar"]), int(sequence["W_lidar"])
        if tuple(images.shape[1:3]) != (H, W) or tuple(poses.shape) != (images.shape[0], 4, 4):
            raise ValueError(f"LidarBatchSampler: {tuple(images.shape)} images and {tuple(poses.shape)} poses do not make a "
                             f"sequence of {H} x {W} frames")
        if poses.dtype != torch.float32:
            raise ValueError(f"LidarBatchSampler: poses_lidar must be float32, got {poses.dtype}")
        if int(seed) < 0 or int(seed) >= 1 << 64 or int(stream_id) < 0 or int(stream_id) >= 1 << 31:
            raise ValueError("LidarBatchSampler: seed must fit 64 bits and stream_id 31, neither negative")
        _hip.require_symbols(("lnh_lidar_sample_batch", "lnh_lidar_frame_rays"), "LidarBatchSampler")
        self.poses, self.images = poses.contiguous(), images.contiguous()
        self._dtype = _hip.dtype_code(images.dtype)
        self.F, self.H, self.W = int(images.shape[0]), H, W
        self.intrinsics = (float(intrinsics[0]), float(intrinsics[1]))
        self.seed, self.stream_id, self.epoch = int(seed), int(stream_id), 0
        self.uid = next(_UIDS)  # (the captured steps are keyed on it: an id() could be reused after a collection)
        dev = poses.device
        self.perm = torch.arange(self.F, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=dev)
        self.set_patch(num_rays, patch_size)

    # ---- geometry of a batch
    def set_patch(self, num_rays, patch_size):
        """Another batch size / patch shape from here on (the reference's --change_patch_size_lidar): the output buffers
        are allocated anew, nothing else changes — cursor, frame order and random stream go on."""
        px, py = patch_shape(patch_size)
        if int(num_rays) <= 0:
            raise ValueError(f"LidarBatchSampler: num_rays must be positive, got {num_rays}")
        if px > 0 and (py <= 0 or px >= self.H or py >= self.W):
            raise ValueError(f"LidarBatchSampler: a {px} x {py} patch does not leave a corner to draw in a {self.H} x {self.W} "
                             "image (0 < px < H and 0 < py < W; the reference's randint raises on the empty range)")
        n = batch_rows(num_rays, self.H, self.W, px, py)
        if n == 0:
            raise ValueError(f"LidarBatchSampler: num_rays {num_rays} is less than one {px} x {py} patch")
        self.num_rays, self.px, self.py, self.n = int(num_rays), px, py, n
        dev = self.poses.device
        self.rays_o = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self.rays_d = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self.gt = torch.empty((n, 3), dtype=self.images.dtype, device=dev)
        self.inds = torch.empty(n, dtype=torch.int32, device=dev)

    @property
    def patch(self):
        """The `patch` argument of LidarTrainer.step for these batches."""
        return (self.px, self.py) if self.px > 1 else (1, 1)

    def graph_key(self):
        """Everything a captured draw bakes in as kernel arguments."""
        return (self.uid, self.n, self.px, self.py, self.F, self.H, self.W, self.intrinsics, self.seed, self.stream_id,
                self.images.dtype, self.poses.data_ptr(), self.images.data_ptr())

    # ---- drawing
    def draw_into(self, rays_o, rays_d, gt, inds, frame=-1):
        """The two launches (draw, advance) on the current stream, writing the caller's [n,3] / [n] buffers.  frame: -1 = the
        epoch's next frame, perm[step % F]; an index = that frame (the counters advance all the same)."""
        _hip.call("lnh_lidar_sample_batch", self.poses.data_ptr(), self.images.data_ptr(), self._dtype, self.F, self.H,
                  self.W, self.intrinsics[0], self.intrinsics[1], self.perm.data_ptr(), self.cursor.data_ptr(),
                  self.seed & 0xFFFFFFFF, self.seed >> 32, self.stream_id, self.num_rays, self.px, self.py, int(frame),
                  rays_o.data_ptr(), rays_d.data_ptr(), gt.data_ptr(), inds.data_ptr())

    def draw(self, frame=-1):
        """One batch: (rays_o [1,n,3], rays_d [1,n,3], images_lidar [1,n,3]) — VIEWS of the sampler's own static buffers,
        rewritten in place by the next draw (self.inds [n] likewise): use them before drawing again, clone what must last."""
        self.draw_into(self.rays_o, self.rays_d, self.gt, self.inds, frame)
        return self.rays_o[None], self.rays_d[None], self.gt[None]

    def new_epoch(self):
        """A fresh frame order, written into the static `perm` tensor (one small host-to-device copy, never inside a
        graph), and the in-epoch step back to 0.  The order comes from a host generator seeded by (seed, epoch, stream_id)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LidarBatchSampler.new_epoch(): not while a stream is capturing")
        self.epoch += 1
        self.perm.copy_(torch.from_numpy(self._permutation(self.epoch)))
        self.cursor[:1].zero_()

    def _permutation(self, epoch):
        rng = np.random.default_rng([self.seed & 0xFFFFFFFF, self.seed >> 32, int(epoch), self.stream_id])
        return rng.permutation(self.F).astype(np.int32)

    # ---- evaluation frames
    def frame(self, i):
        """Frame i as LidarTrainer.eval_step's `data`: rays_o_lidar / rays_d_lidar [1, H*W, 3] (lnh_lidar_frame_rays),
        images_lidar [1, H, W, 3] (a view of the sequence), H_lidar, W_lidar."""
        i = int(i)
        if not 0 <= i < self.F:
            raise IndexError(f"LidarBatchSampler.frame({i}): the sequence has {self.F} frames")
        dev = self.poses.device
        rays_o = torch.empty((1, self.H * self.W, 3), dtype=torch.float32, device=dev)
        rays_d = torch.empty_like(rays_o)
        _hip.call("lnh_lidar_frame_rays", self.poses.data_ptr(), self.F, i, self.H, self.W, self.intrinsics[0],
                  self.intrinsics[1], rays_o.data_ptr(), rays_d.data_ptr())
        return {"rays_o_lidar": rays_o, "rays_d_lidar": rays_d, "images_lidar": self.images[i:i + 1], "H_lidar": self.H,
                "W_lidar": self.W}

    def frames(self):
        """Every frame of the sequence in file order (LidarTrainer.evaluate's `frames`)."""
        for i in range(self.F):
            yield self.frame(i)

    def __len__(self):
        return self.F

    # ---- state
    def state_dict(self):
        """Seed, stream, epoch, both counters and the frame order: a sampler that loads it continues with the identical
        sequence of batches.  Reads the cursor back (synchronises).  Kept apart from the trainer's checkpoint, whose layout is
        the reference's."""
        step, draws = (int(v) for v in self.cursor.tolist())
        return {"seed": self.seed, "stream_id": self.stream_id, "epoch": self.epoch, "step": step, "draws": draws,
                "perm": self.perm.cpu().clone()}

    def load_state_dict(self, sd):
        perm = torch.as_tensor(sd["perm"]).to(torch.int32).reshape(-1)
        if perm.numel() != self.F or int(perm.min()) < 0 or int(perm.max()) >= self.F:
            raise ValueError(f"LidarBatchSampler.load_state_dict: the saved frame order does not fit a sequence of {self.F} frames")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LidarBatchSampler.load_state_dict(): not while a stream is capturing")
        # (seed and stream are kernel arguments of a captured draw: graph_key() moves with them, the step is captured anew)
        self.seed, self.stream_id, self.epoch = int(sd["seed"]), int(sd["stream_id"]), int(sd["epoch"])
        self.perm.copy_(perm)
        self.cursor.copy_(torch.tensor([int(sd["step"]), int(sd["draws"])], dtype=torch.int64))
