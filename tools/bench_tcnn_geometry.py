#!/usr/bin/env python3
"""Training-step time of the tcnn-shaped network (network_tcnn.NeRFNetwork, fused LiDAR chain, fp16) in its two hash-grid
level geometries: "torch-ngp" (the default) and "tcnn" (tiny-cuda-nn's lattice, kernel gridtype 2).  Same rays for both,
4096 rays x (768 + 64) samples, HIP-event time of forward + backward per step, median after warm-up.

    python tools/bench_tcnn_geometry.py [--steps 30] [--warmup 10] [--rays 4096] [--only tcnn|torch-ngp]

(--only: one geometry, once — for a per-kernel trace of one geometry under a profiler.)

Prints one JSON line: ms per step of each geometry and the ratio tcnn / torch-ngp.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lidar-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SCALE = 0.010784853507573345


def step_times(geometry, o, d, gt, steps, warmup):
    from lidarnerf.nerf import fused
    from lidarnerf.nerf.network_tcnn import NeRFNetwork
    from lidarnerf.nerf.train_step import lidar_loss
    torch.manual_seed(0)
    net = NeRFNetwork(encoding="hashgrid", desired_resolution=32768, log2_hashmap_size=19, bound=1, min_near=SCALE,
                      min_near_lidar=SCALE, tcnn_geometry=geometry).cuda().train()
    with torch.no_grad():
        net.encoder.impl.params.uniform_(-0.3, 0.3)
    if not fused.supported(net, True, 768, 64):
        raise RuntimeError(f"geometry {geometry}: the fused chain does not serve this model")
    times = []
    for s in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.render(o, d, cal_lidar_color=True, staged=False, perturb=False, num_steps=768, upsample_steps=64)
            loss, _, _ = lidar_loss(out, gt)
        loss.backward()
        b.record()
        b.synchronize()
        if s >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.percentile(times, 25)), float(np.percentile(times, 75))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--only", choices=("torch-ngp", "tcnn"), default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(1)
    N = a.rays
    o = ((torch.rand(N, 3, generator=g) - 0.5) * 0.1).cuda()[None]
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda()[None]
    gt = torch.rand(1, N, 3, generator=g).cuda()
    gt[..., 0] = (gt[..., 0] > 0.2).float()
    res = {"rays": N, "samples": 768 + 64, "steps": a.steps, "warmup": a.warmup}
    order = (a.only,) if a.only else ("torch-ngp", "tcnn", "torch-ngp", "tcnn")  # interleaved twice: drift shows as a spread
    for geometry in order:
        med, q1, q3 = step_times(geometry, o, d, gt, a.steps, a.warmup)
        res.setdefault(geometry, []).append({"ms_median": round(med, 3), "ms_q1": round(q1, 3), "ms_q3": round(q3, 3)})
    if a.only:
        print(json.dumps(res))
        return
    best = {k: min(r["ms_median"] for r in res[k]) for k in ("torch-ngp", "tcnn")}
    res["ratio_tcnn_over_torch_ngp"] = round(best["tcnn"] / best["torch-ngp"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
