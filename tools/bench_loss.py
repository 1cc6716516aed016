#!/usr/bin/env python3
"""Cost of the loss options: the loss launch alone and the captured training step, default options against the heaviest.

    python tools/bench_loss.py [--iters 200] [--steps 30] [--warmup 10]

Loss launch: lnh_lidar_loss_patch (the default set on 2x8 patches) and lnh_lidar_loss_ex (the heaviest set: huber depth,
bce ray-drop, l1 intensity, Sobel + cos gradient term, all three smoothness terms) at 4096 and 16384 rays; `--iters`
calls captured in one hipGraph, HIP-event time of its replays divided by the number of calls (forward + the gradients it
writes; backward is a view).
Step: LidarTrainer(graph=True) at the benchmark's shape (4096 rays x (768 + 64) samples, 2x8 patch epochs), median
HIP-event time of a replayed step, default against heaviest, interleaved twice.

Prints one JSON line.
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

HEAVY = dict(depth_loss="huber", raydrop_loss="bce", intensity_loss="l1", depth_grad_loss="cos", sobel_grad=True,
             grad_norm_smooth=True, spatial_smooth=True, tv_loss=True)


def loss_us(N, options, iters):
    import bench
    from lidarnerf.nerf.train_step import fused_lidar_loss
    g = torch.Generator().manual_seed(N)
    gt = torch.rand(1, N, 3, generator=g)
    gt[..., 0] = (gt[..., 0] > 0.2).float()
    gt[..., 2] = bench.SCALE * (5.0 + 60.0 * gt[..., 2])
    gt = gt.cuda()
    out = {"depth_lidar": (gt[..., 2] * 1.01).contiguous(), "image_lidar": torch.rand(1, N, 2, generator=g).cuda()}
    patch = (2, 8, bench.SCALE, 100.0)
    run = lambda: fused_lidar_loss(out, gt, 1000.0, 1.0, 10.0, patch=patch, options=options, scale=bench.SCALE)  # noqa: E731
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    # `iters` calls captured in one graph and replayed: GPU time only (a Python loop of calls is bound by the host)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            run()
    graph.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (5 * iters)


def step_ms(options, steps, warmup):
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=True,
                      render_kwargs=dict(num_steps=768, upsample_steps=64), loss_options=options)
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, 4096, 0, dev, (2, 8), "analytic") for s in range(8)]
    times = []
    for s in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step(*batches[s % 8], patch=(2, 8))
        b.record()
        b.synchronize()
        if s >= warmup:
            times.append(a.elapsed_time(b))
    if not tr.graph:
        raise RuntimeError(f"the step was not captured: {tr.graph_error}")
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    from lidarnerf.nerf.train_step import LidarLossOptions
    torch.cuda.set_device(0)
    heavy = LidarLossOptions(**HEAVY)
    res = {"loss_us": {}, "step_ms": {"default": [], "heaviest": []}}
    for N in (4096, 16384):
        res["loss_us"][f"default_{N}"] = round(loss_us(N, None, a.iters), 2)
        res["loss_us"][f"heaviest_{N}"] = round(loss_us(N, heavy, a.iters), 2)
    for _ in range(2):
        res["step_ms"]["default"].append(round(step_ms(None, a.steps, a.warmup), 3))
        res["step_ms"]["heaviest"].append(round(step_ms(heavy, a.steps, a.warmup), 3))
    best = {k: min(v) for k, v in res["step_ms"].items()}
    res["step_ratio_heaviest_over_default"] = round(best["heaviest"] / best["default"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
