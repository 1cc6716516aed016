#!/usr/bin/env python3
"""G12 — BASELINE config 1 through the reference's OWN renderer (CPU): NeRFRenderer.run (lidarnerf/nerf/renderer.py:99-298)
with the pure-torch FreqEncoder of encoding.py:6-47 and trunc_exp (activation.py:6-20), wired as network.py:162-237 wires
them, on the weights of oracle.render_ref.RefFreqField (seed 3).  Stores the weights, the rays, the ground truth, the
reference's depth / image / weights_sum and the gradient of the LiDAR loss of those outputs w.r.t. every weight, so that
tests/test_config1_cpu.py checks oracle.render_ref.run_lidar (what bench.py times as `cpu_baseline`) without the
reference checkout.

    python tests/golden/make_g12_config1_freq.py /path/to/lidar-nerf     # writes tests/golden/g12_config1_freq.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SCALE = 0.010784853507573345


def main(ref):
    sys.path.insert(0, ROOT)
    from oracle import render_ref
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))  # visualisation-only import in the reference
    sys.path.insert(0, ref)
    from lidarnerf.activation import trunc_exp
    from lidarnerf.encoding import FreqEncoder
    from lidarnerf.nerf.renderer import NeRFRenderer

    torch.manual_seed(3)
    ours = render_ref.RefFreqField()

    class RefNet(NeRFRenderer):  # network.py:162-237 with the pure-torch encoders (encoding.py:67: the commented line)
        def __init__(self):
            super().__init__(bound=1, min_near=SCALE, min_near_lidar=SCALE)
            self.enc = FreqEncoder(input_dim=3, max_freq_log2=5, N_freqs=6, log_sampling=True)
            self.enc_dir = FreqEncoder(input_dim=3, max_freq_log2=11, N_freqs=12, log_sampling=True)
            self.out_dim = self.out_lidar_color_dim = 2

        def density(self, x):
            h = torch.relu(ours.sigma_net[0](self.enc(x, bound=self.bound)))
            h = ours.sigma_net[1](h)
            return {"sigma": trunc_exp(h[..., 0]), "geo_feat": h[..., 1:]}

        def color(self, x, d, cal_lidar_color=False, mask=None, geo_feat=None, **kw):
            rgbs = torch.zeros(mask.shape[0], self.out_dim, dtype=x.dtype)
            if not mask.any():
                return rgbs
            h = torch.cat([self.enc_dir(d[mask]), geo_feat[mask]], dim=-1)
            for i, lin in enumerate(ours.lidar_color_net):
                h = lin(h)
                if i != 2:
                    h = torch.relu(h)
            rgbs[mask] = torch.sigmoid(h)
            return rgbs

    ref_net = RefNet().eval()
    g = torch.Generator().manual_seed(5)
    n = 24
    o = (torch.rand(n, 3, generator=g) - 0.5) * 0.02
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    want = ref_net.run(o, d, cal_lidar_color=True, num_steps=768, upsample_steps=64, perturb=False)
    gt = torch.rand(n, 3, generator=g)
    out = {"rays_o": o.numpy(), "rays_d": d.numpy(), "gt": gt.numpy()}
    for name, p in ours.named_parameters():
        out["w_" + name] = p.detach().numpy().copy()
    for k in ("depth_lidar", "image_lidar", "weights_sum_lidar"):
        out[k] = want[k].detach().numpy()
    # the reference renders a flat batch: the loss sees the shapes run_lidar returns ([N], [N, 2])
    ours.zero_grad(set_to_none=True)
    render_ref.lidar_loss(want["depth_lidar"].reshape(n), want["image_lidar"].reshape(n, 2), gt).backward()
    for name, p in ours.named_parameters():
        out["grad_" + name] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "g12_config1_freq.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
