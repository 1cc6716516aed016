#!/usr/bin/env python3
"""What the ray-ordered marcher costs, the two sides alternating window by window IN ONE PROCESS on the NeRF-MVL-shaped
occupancy-grid workload of `bench.py --workload nerfmvl` (256 x 1800 frames, 4096 rays) after its settling steps:

    marcher   lnh_march_rays_train (one launch, rows in workgroup-arrival order) against lnh_march_rays_train_ordered (count,
              one-workgroup scan, write: three launches, rows in ray order) on the settled occupancy grid — a training batch
              of 4096 rays and one whole frame of 256 x 1800 rays; device time per call from HIP events around a window
    step      LidarTrainer.step_sampled(graph=True) with model.ordered_march off against on: ONE trainer, one model, the flag
              flipped between windows (the captured steps are keyed on it); wall time per step, windows ending in a synchronise

    python tools/bench_march_ordered.py [--rounds 7] [--window 0.5] [--out profiles/march_ordered_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

NAMES = {"arrival": "lnh_march_rays_train", "ordered": "lnh_march_rays_train_ordered"}


def summary(v):
    return f"{statistics.median(v):9.3f}   (min {min(v):.3f}, max {max(v):.3f}; " + ", ".join(f"{x:.3f}" for x in v) + ")"


def against(a, b, what, unit):
    d = [y - x for x, y in zip(a, b)]
    return (f"  ordered against {what}, window by window: " + ", ".join(f"{x:+.3f}" for x in d) +
            f" {unit}  ->  median {statistics.median(d):+.3f} {unit}, slower in {sum(x > 0 for x in d)} of {len(d)} windows")


def bench_marchers(model, rays_o, rays_d, title, args, lines, calls=100):
    """Device time per call of the two entry points on the same rays and the model's current bitfield."""
    from lidarnerf import _hip, raymarching
    N, dev = rays_o.shape[0], rays_o.device
    nears = torch.full((N,), float(model.min_near_lidar), device=dev)
    _, far_box = raymarching.near_far_from_aabb(rays_o, rays_d, model.aabb_train, model.min_near_lidar)
    fars = torch.minimum(nears * 81.0, far_box)
    noises = torch.zeros(N, device=dev)
    bits = model.density_bitfield.contiguous()
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    rays = torch.zeros((N, 3), dtype=torch.int32, device=dev)

    def march(name, M, bufs):
        _hip.zero_regions([counter])
        _hip.call(NAMES[name], rays_o.data_ptr(), rays_d.data_ptr(), bits.data_ptr(), float(model.bound), 0.0, 1024, N,
                  model.cascade, model.grid_size, M, nears.data_ptr(), fars.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                  bufs[2].data_ptr(), rays.data_ptr(), counter.data_ptr(), noises.data_ptr())

    tiny = [torch.zeros(8, device=dev) for _ in range(3)]
    march("ordered", 1, tiny)  # (M = 1: counts only, nothing is written)
    total = int(counter[0])
    M = total + 128
    bufs = [torch.zeros((M, 3), device=dev), torch.zeros((M, 3), device=dev), torch.zeros((M, 2), device=dev)]

    def window(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            march(name, M, bufs)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    for name in NAMES:
        window(name)
    times = {k: [] for k in NAMES}
    for _ in range(args.rounds):
        for name in NAMES:
            times[name].append(window(name))
    lines.append(f"{title}: {N} rays, {total} samples ({total / N:.1f} per ray); us of device time per call (a 1-launch clear of "
                 f"the counter included on both sides), windows of {calls} calls, the two sides alternating, {args.rounds} rounds")
    for name in NAMES:
        lines.append(f"  {NAMES[name]:<30s} {summary(times[name])}")
    lines.append(against(times["arrival"], times["ordered"], "arrival order", "us"))


def bench_steps(trainer, sampler, args, lines):
    model = trainer.model

    def window(flag):
        model.ordered_march = flag
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < args.window:
            for _ in range(16):
                trainer.step_sampled(sampler)
                n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, n

    for flag in (False, True):  # both sides captured at the current rung of the capacity ladder
        window(flag)
    times, steps = {False: [], True: []}, {}
    for _ in range(args.rounds):
        for flag in (False, True):
            ms, steps[flag] = window(flag)
            times[flag].append(ms)
    lines.append(f"occupancy training step (step_sampled, graph mode {'on' if trainer.graph else 'OFF: ' + str(trainer.graph_error)}, "
                 f"{len(trainer._graphs)} captured steps): ms of wall time per step, windows of >= {args.window} s ending in a "
                 f"synchronise (a grid update every 16th step on both sides), the two sides alternating, {args.rounds} rounds")
    for flag in (False, True):
        lines.append(f"  ordered_march = {str(flag):<14s} {summary(times[flag])}   ~{steps[flag]} steps per window")
    lines.append(against(times[False], times[True], "ordered_march = False", "ms"))
    model.ordered_march = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--settle", type=int, default=320)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_march_ordered: no GPU — nothing is measured without one")
    from bench_sampler import nerfmvl_sequence
    from lidarnerf.dataset.sampler import LidarBatchSampler
    from lidarnerf.nerf.network import NeRFNetwork
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    scale, H, W, intr = 0.005, 256, 1800, (15.0, 40.0)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", desired_resolution=32768, log2_hashmap_size=19, num_layers=2, hidden_dim=64,
                        geo_feat_dim=15, bound=1, density_scale=1, min_near=scale, min_near_lidar=scale, density_thresh=10,
                        bg_radius=-1, cuda_ray=True).to(dev).train()
    trainer = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=scale, graph=True)
    sampler = LidarBatchSampler(nerfmvl_sequence(dev, scale, H, W, intr), intr, num_rays=4096, patch_size=1, seed=0)
    for _ in range(args.settle):  # the occupancy grid settles (bench.py --workload nerfmvl does the same before it measures)
        trainer.step_sampled(sampler)
    torch.cuda.synchronize()
    lines = [f"ray-ordered marcher against the arrival-order marcher, NeRF-MVL-shaped workload after {args.settle} settling steps "
             f"({torch.cuda.get_device_name(0)})"]
    o, d, _ = sampler.draw()
    bench_marchers(model, o[0].clone(), d[0].clone(), "training batch", args, lines)
    frame = sampler.frame(0)
    bench_marchers(model, frame["rays_o_lidar"][0].contiguous(), frame["rays_d_lidar"][0].contiguous(),
                   f"whole frame ({H} x {W})", args, lines, calls=20)
    bench_steps(trainer, sampler, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
