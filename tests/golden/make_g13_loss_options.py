#!/usr/bin/env python3
"""G13: the reference's Trainer.train_step loss under every loss option of its CLI (CPU).

    python tests/golden/make_g13_loss_options.py <reference checkout>

The G8 recipe (make_golden.py g8) with the options varied: the reference's OWN Trainer.train_step
(lidarnerf/nerf/utils.py:697-884), called unbound on a stub `self` whose criterion dict is built the way
main_lidarnerf.py:330-342 builds it from the CLI's options, and whose model.render returns leaf tensors.  Writes
g13_loss_options.npz next to this script: the inputs (two batches: 512 rays and 4096 rays), and per case the loss and
d loss / d (depth, image).  `cases` is a JSON list of {name, batch, patch, options}; `options` uses the CLI's names.

Cases: every criterion in every slot on the per-ray path; every depth_grad_loss with and without sobel_grad on 2x8 and
4x4 patches; each smoothness term alone in both Sobel modes; all terms together with grad_loss on and off; the heaviest
set on 4096 rays.  The 512-ray batch holds dropped rays, two wholly dropped patches (rays 48-63, 160-175: all-zero
masked vectors for `cos`), equal neighbouring predictions (|dx| = 0), and ground-truth neighbours on both sides of the
0.01 m mask threshold.  (No patch of constant prediction: its interior Sobel response is zero only by cancellation, and
the sign the reference's conv2d rounds it to is not a property of the loss.)
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
ALPHAS = dict(alpha_d=1000.0, alpha_r=1.0, alpha_i=10.0, alpha_grad=100.0)  # configs/kitti360_1908.txt:2-5
DEFAULTS = dict(depth_loss="l1", raydrop_loss="mse", intensity_loss="mse", depth_grad_loss="l1", grad_loss=True,
                sobel_grad=False, grad_norm_smooth=False, spatial_smooth=False, tv_loss=False, alpha_grad_norm=1.0,
                alpha_spatial=0.1, alpha_tv=1.0)


def make_batch(N, seed):
    """images_lidar [1, N, 3] (raydrop, intensity, depth in scene units), depth [N], image [N, 2]."""
    g = torch.Generator().manual_seed(seed)
    raydrop = (torch.rand(N, generator=g) < 0.8).float()
    intensity = torch.rand(N, generator=g)
    # ground truth in metres along rows of 8 (= two rows of a 4x4 patch): steps of 2-8 mm or 12-20 mm, either sign —
    # neighbours on both sides of the 0.01 m threshold, none within 2 mm of it
    small = torch.rand(N // 8, 8, generator=g) < 0.5
    mag = torch.where(small, 0.002 + 0.006 * torch.rand(N // 8, 8, generator=g),
                      0.012 + 0.008 * torch.rand(N // 8, 8, generator=g))
    sign = torch.where(torch.rand(N // 8, 8, generator=g) < 0.5, -1.0, 1.0)
    metres = (5.0 + 60.0 * torch.rand(N // 8, 1, generator=g) + (sign * mag).cumsum(-1)).reshape(N)
    # predictions: a few per cent off on half of the rays, within a fraction of a per cent on the other half (both sides
    # of the huber delta 0.2 * scale)
    rel = torch.where(torch.rand(N, generator=g) < 0.5, 0.05, 0.0005)
    depth = SCALE * metres * (1 + rel * torch.randn(N, generator=g))
    image = torch.rand(N, 2, generator=g)
    near = torch.rand(N, generator=g) < 0.25  # ray-drop / intensity predictions close to the truth
    image[:, 0] = torch.where(near, raydrop + 0.001 * torch.randn(N, generator=g), image[:, 0])
    image[:, 1] = torch.where(near, intensity + 0.001 * torch.randn(N, generator=g), image[:, 1])
    if N == 512:
        raydrop[48:64] = 0.0
        raydrop[160:176] = 0.0
        for n in (1, 9, 17, 34, 130, 201, 258, 306, 401, 449):  # (n, n + 1) in one row of 8 and of 4
            depth[n + 1] = depth[n]
            raydrop[n] = raydrop[n + 1] = 1.0
    gt = torch.stack([raydrop, intensity, SCALE * metres], -1)[None]
    return gt, depth, image


def cases():
    out = []

    def add(name, batch, patch, **opts):
        out.append(dict(name=name, batch=batch, patch=patch, options=dict(DEFAULTS, **opts)))

    # per ray: every criterion in every slot
    add("ray_default", 512, [1, 1])
    add("ray_mse_l1_huber", 512, [1, 1], depth_loss="mse", raydrop_loss="l1", intensity_loss="huber")
    add("ray_huber_bce_bce", 512, [1, 1], depth_loss="huber", raydrop_loss="bce", intensity_loss="bce")
    add("ray_bce_huber_l1", 512, [1, 1], depth_loss="bce", raydrop_loss="huber", intensity_loss="l1")
    for patch in ([2, 8], [4, 4]):
        tag = f"{patch[0]}x{patch[1]}"
        for crit in ("l1", "mse", "huber", "bce", "cos"):
            for sobel in (False, True):
                add(f"grad_{crit}{'_sobel' if sobel else ''}_{tag}", 512, patch, depth_grad_loss=crit, sobel_grad=sobel)
        for flag in ("grad_norm_smooth", "spatial_smooth", "tv_loss"):
            for sobel in (False, True):
                add(f"{flag}{'_sobel' if sobel else ''}_{tag}", 512, patch, grad_loss=False, sobel_grad=sobel, **{flag: True})
        for grad in (True, False):
            for sobel in (False, True):
                add(f"all{'_grad' if grad else ''}{'_sobel' if sobel else ''}_{tag}", 512, patch, depth_loss="huber",
                    raydrop_loss="bce", intensity_loss="l1", depth_grad_loss="cos" if sobel else "huber", grad_loss=grad,
                    sobel_grad=sobel, grad_norm_smooth=True, spatial_smooth=True, tv_loss=True, alpha_grad_norm=0.5,
                    alpha_spatial=0.3, alpha_tv=2.0)
    add("heavy_4096_2x8", 4096, [2, 8], depth_loss="huber", raydrop_loss="bce", intensity_loss="l1",
        depth_grad_loss="cos", sobel_grad=True, grad_norm_smooth=True, spatial_smooth=True, tv_loss=True)
    add("ray_4096", 4096, [1, 1], depth_loss="huber", raydrop_loss="bce", intensity_loss="mse")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference project")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from make_golden import _reference_trainer  # (the G8 stubs of the imports train_step never touches)
    Trainer = _reference_trainer()
    torch.set_num_threads(4)
    batches = {512: make_batch(512, 1313), 4096: make_batch(4096, 4096)}
    out = {}
    for N, (gt, depth, image) in batches.items():
        out[f"b{N}_gt"], out[f"b{N}_depth"], out[f"b{N}_image"] = gt[0].numpy(), depth.numpy(), image.numpy()
    all_cases = cases()
    for c in all_cases:
        gt, depth0, image0 = batches[c["batch"]]
        N = c["batch"]
        depth = depth0.clone()[None].requires_grad_(True)   # depth_lidar [1, N]
        image = image0.clone()[None].requires_grad_(True)   # image_lidar [1, N, 2]

        class _Model:
            def render(self, rays_o, rays_d, **kw):
                return {"image_lidar": image, "depth_lidar": depth}

        o = c["options"]
        patch = 1 if c["patch"] == [1, 1] else c["patch"]
        opt = argparse.Namespace(enable_lidar=True, patch_size=1, patch_size_lidar=patch, scale=SCALE, **ALPHAS, **o)
        loss_dict = {  # main_lidarnerf.py:330-342
            "mse": torch.nn.MSELoss(reduction="none"),
            "l1": torch.nn.L1Loss(reduction="none"),
            "bce": torch.nn.BCEWithLogitsLoss(reduction="none"),
            "huber": torch.nn.HuberLoss(reduction="none", delta=0.2 * opt.scale),
            "cos": torch.nn.CosineSimilarity(),
        }
        criterion = {"depth": loss_dict[opt.depth_loss], "raydrop": loss_dict[opt.raydrop_loss],
                     "intensity": loss_dict[opt.intensity_loss], "grad": loss_dict[opt.depth_grad_loss]}
        me = types.SimpleNamespace(opt=opt, model=_Model(), criterion=criterion, device=torch.device("cpu"))
        data = {"rays_o_lidar": torch.zeros(1, N, 3), "rays_d_lidar": torch.zeros(1, N, 3), "images_lidar": gt}
        loss = Trainer.train_step(me, data)[4]
        loss.backward()
        name = c["name"]
        out[f"{name}_loss"] = loss.detach().numpy()
        out[f"{name}_grad_depth"] = depth.grad[0].numpy().copy()
        out[f"{name}_grad_image"] = image.grad[0].numpy().copy()
        print(f"{name:28s} loss {loss.item():.6g}  max|g_depth| {depth.grad.abs().max().item():.3g}")
    data = {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}
    data.update(cases=np.array(json.dumps(all_cases)), scale=np.float32(SCALE),
                alphas=np.array([ALPHAS[k] for k in ("alpha_d", "alpha_r", "alpha_i", "alpha_grad")], dtype=np.float32))
    path = os.path.join(HERE, "g13_loss_options.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
