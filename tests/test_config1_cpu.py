"""BASELINE config 1 (freq encoder + plain PyTorch MLP on the CPU): oracle.render_ref.RefFreqField + run_lidar — what
bench.py times as `cpu_baseline` — against the reference (NeRFRenderer.run with the pure-torch FreqEncoder of
encoding.py:6-47 and nn.Linear stacks wired as network.py:162-237 wires them).  The reference's outputs and weight
gradients are the golden vector G12 (tests/golden/make_g12_config1_freq.py)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_config1_freq.npz")


def test_freq_field_matches_imported_reference():
    from oracle import render_ref
    z = np.load(GOLDEN)
    scale = 0.010784853507573345
    ours = render_ref.RefFreqField()
    with torch.no_grad():
        for name, p in ours.named_parameters():
            p.copy_(torch.from_numpy(z["w_" + name]))
    o, d, gt = (torch.from_numpy(z[k]) for k in ("rays_o", "rays_d", "gt"))
    got = render_ref.run_lidar(o, d, ours.density, ours.color, torch.tensor([-1.0, -1, -1, 1, 1, 1]), scale, 768, 64)
    for k in ("depth_lidar", "image_lidar", "weights_sum_lidar"):
        np.testing.assert_allclose(got[k].detach().numpy(), z[k].reshape(got[k].shape), rtol=1e-5, atol=1e-7)
    # gradients of the scalar the trainer differentiates
    ours.zero_grad(set_to_none=True)
    render_ref.lidar_loss(got["depth_lidar"], got["image_lidar"], gt).backward()
    for name, p in ours.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), z["grad_" + name], rtol=2e-4, atol=1e-6)
