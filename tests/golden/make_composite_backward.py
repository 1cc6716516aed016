#!/usr/bin/env python3
"""Records what lnh_lidar_composite_backward of the built library writes (needs the GPU) into
tests/golden/composite_backward_parent.npz: inputs AND outputs, K = 2, N = 5 rays at T = 1, 63, 65, 449 — once as the
training step calls it (grad_weights_sum and grad_rgb null) and once with both.

    LNH_LIB_PATH=<library of the commit before csrc/composite_adjoint.h> python tests/golden/make_composite_backward.py [out.npz]

The record is a statement about THAT build: tests/test_train_tail_gpu.py holds later libraries to its bits, so it is
regenerated only when a change means to alter the compositing adjoint, from a build of the commit before that change.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "lidar-nerf_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from gpu_util import call  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "composite_backward_parent.npz")
    rec, i, N = {}, 0, 5
    for T in (1, 63, 65, 449):
        r = np.random.default_rng(77 + T)
        z = np.sort(r.uniform(0.01, 0.81, (N, T)).astype(np.float32), axis=1)
        sigma = r.uniform(0.0, 3.0, (N, T)).astype(np.float32)
        sigma[0] = 0.0                           # a ray without any weight
        sigma[1, :min(T, 8)] = 40.0 * T          # opaque within its first samples
        rgb = r.uniform(0.0, 1.0, (N, T, 2)).astype(np.float32)
        rgb[2, T // 2:] = 0.0                    # colour 0, as behind the mask threshold
        inp = dict(z=z, sigma=sigma, rgb=rgb, sd=np.full(N, 0.8 / T, np.float32),
                   g_ws=r.standard_normal(N).astype(np.float32), g_depth=(r.standard_normal(N) * 200).astype(np.float32),
                   g_image=r.standard_normal((N, 2)).astype(np.float32))
        inp["g_depth"][3] = 0.0                  # sign(0) = 0: no depth gradient
        d = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
        for full in (False, True):
            gs = torch.full((N, T), float("nan"), device="cuda")
            gc = torch.full((N, T, 2), float("nan"), device="cuda")
            call("lnh_lidar_composite_backward", d["g_ws"] if full else None, d["g_depth"], d["g_image"], d["z"], d["sigma"],
                 d["rgb"], d["sd"], N, T, 2, 1.0, gs, gc if full else None)
            torch.cuda.synchronize()
            assert torch.isfinite(gs).all() and (not full or torch.isfinite(gc).all())
            for k, v in inp.items():
                rec[f"{i}_{k}"] = v
            rec[f"{i}_full"] = np.array(full)
            rec[f"{i}_out_g_sigma"] = gs.cpu().numpy()
            rec[f"{i}_out_g_rgb"] = gc.cpu().numpy() if full else np.zeros((0,), np.float32)
            i += 1
    rec["n_cases"] = np.array(i)
    np.savez_compressed(out, **rec)
    print(f"{out}: {i} cases, {os.path.getsize(out)} bytes")
