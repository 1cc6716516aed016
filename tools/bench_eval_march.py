#!/usr/bin/env python3
"""Full-frame occupancy-grid EVALUATION: the existing path (run_cuda in eval mode: lnh_march_rays_train over every ray to
its far end, field on every occupied sample) against the alive-ray loop (run_cuda_alive), same process, same trained model.

Scene = bench.py run_nerfmvl (restated here: a 2 m sphere seen from a 6 m ring, 256 x 1800 range image, intrinsics (15, 40),
scale 0.005, the same NeRFNetwork(cuda_ray=True)), trained with LidarTrainer.step for the same 320 settling steps.  One frame
= the rays inside the object's bounding sphere, render(staged=True, max_ray_batch=4096) under fp16 autocast.

    python tools/bench_eval_march.py [--repeats 7] [--n-step0 16 [8 32 ...]] [--out profiles/eval_march.json]

Times are synchronised wall time per frame, medians over --repeats after --warmup frames of each path, the two paths
alternating.  No speed-up is assumed: the ratio is reported whatever it is."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lidar-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train-steps", type=int, default=320)
    ap.add_argument("--rays", type=int, default=4096, help="rays per training step")
    ap.add_argument("--max-ray-batch", type=int, default=4096)
    ap.add_argument("--n-step0", type=int, nargs="+", default=[16], help="first-round samples per ray; the first is the headline")
    ap.add_argument("--only", choices=["existing", "alive"], help="render one path only (for a profiler run of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_march.json"))
    args = ap.parse_args()
    from lidarnerf import _hip, raymarching
    from lidarnerf.dataset.rays import get_lidar_rays
    from lidarnerf.nerf.network import NeRFNetwork
    from lidarnerf.nerf.train_step import LidarTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_march.py needs a GPU: the HIP extension is the product path (no CPU fallback)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    _hip.lib()
    scale, Himg, Wimg, intr = 0.005, 256, 1800, (15.0, 40.0)
    R, ring = 2.0 * scale, 6.0 * scale
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", desired_resolution=32768, log2_hashmap_size=19, num_layers=2, hidden_dim=64,
                        geo_feat_dim=15, bound=1, density_scale=1, min_near=scale, min_near_lidar=scale,
                        density_thresh=10, bg_radius=-1, cuda_ray=True).to(device).train()
    trainer = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=scale, graph=False)

    def frame(k):
        th = 2 * np.pi * k / 60
        pose = torch.eye(4)
        pose[:3, :3] = torch.tensor([[-np.cos(th), np.sin(th), 0], [-np.sin(th), -np.cos(th), 0], [0, 0, 1.0]])
        pose[:3, 3] = torch.tensor([ring * np.cos(th), ring * np.sin(th), 0.0])
        r = get_lidar_rays(pose[None].to(device), intr, Himg, Wimg, -1)
        o, d = r["rays_o"][0], r["rays_d"][0]
        b = (o * d).sum(-1)
        keep = ((b * b - ((o * o).sum(-1) - (1.2 * R) ** 2)) > 0) & (b < 0)   # inside the object's bounding sphere
        o, d, b = o[keep], d[keep], b[keep]
        disc = b * b - ((o * o).sum(-1) - R * R)
        hit = disc > 0
        depth = torch.where(hit, -b - torch.sqrt(disc.clamp(min=0)), torch.zeros_like(b))
        return o, d, torch.stack([hit.float(), torch.full_like(b, 0.5), depth], -1)

    frames = [frame(k) for k in range(60)]
    for step in range(args.train_steps):
        o, d, gt = frames[step % 60]
        sel = torch.randperm(o.shape[0], generator=torch.Generator(device="cpu").manual_seed(99 + step))[:args.rays].to(device)
        loss = trainer.step(o[sel][None].contiguous(), d[sel][None].contiguous(), gt[sel][None].contiguous())
    torch.cuda.synchronize()
    model.eval()
    o, d, gt = frames[7]
    o, d = o[None].contiguous(), d[None].contiguous()
    n_rays = o.shape[1]

    def render(**kw):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return model.render(o, d, cal_lidar_color=True, staged=True, max_ray_batch=args.max_ray_batch, perturb=False, **kw)

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = render(**kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    variants = {} if args.only == "alive" else {"existing": {}}
    if args.only != "existing":
        for s0 in args.n_step0:
            variants[f"alive_n{s0}"] = {"alive_march": True, "alive_n_step0": s0}
    times, outs = {k: [] for k in variants}, {}
    for i in range(args.warmup + args.repeats):
        for name, kw in variants.items():     # alternating: every path sees the same neighbours on the machine
            ms, outs[name] = timed(**kw)
            if i >= args.warmup:
                times[name].append(ms)
    res = {"scene": "bench.py run_nerfmvl (2 m sphere, 6 m ring, 256 x 1800, intrinsics (15, 40), scale 0.005)",
           "train_steps": args.train_steps, "final_train_loss": float(loss), "frame_rays": n_rays,
           "max_ray_batch": args.max_ray_batch, "repeats": args.repeats, "timing": "synchronised wall time per frame, ms",
           "paths": {}}
    # what each path shades and allocates (untimed passes)
    chunks = [(h, min(h + args.max_ray_batch, n_rays)) for h in range(0, n_rays, args.max_ray_batch)]
    if "existing" in variants:
        marched = 0
        with torch.no_grad():
            for h, t in chunks:
                oc, dc = o[0, h:t].contiguous(), d[0, h:t].contiguous()
                nears, fars = torch.empty(t - h, device=device), torch.empty(t - h, device=device)
                _hip.call("lnh_lidar_march_prologue", oc.data_ptr(), dc.data_ptr(), model.aabb_infer.contiguous().data_ptr(),
                          t - h, float(model.min_near_lidar), 81.0, nears.data_ptr(), fars.data_ptr(), None, None, 0)
                x, _, _, _ = raymarching.march_rays_train(oc, dc, model.bound, model.density_bitfield, model.cascade,
                                                          model.grid_size, nears, fars, None, -1, False, -1, True, 0, 1024)
                marched += x.shape[0]
        res["paths"]["existing"] = {
            "frame_ms_median": float(np.median(times["existing"])), "frame_ms_all": [round(v, 3) for v in times["existing"]],
            "samples_shaded": marched,
            "peak_sample_buffer_bytes": raymarching.march_capacity(min(args.max_ray_batch, n_rays), 1024, -1, 128, True) * 8 * 4}
    for name, kw in variants.items():
        if name == "existing":
            continue
        model.alive_stats_log = []
        render(**kw)
        log, model.alive_stats_log = model.alive_stats_log, None
        entry = {"frame_ms_median": float(np.median(times[name])), "frame_ms_all": [round(v, 3) for v in times[name]],
                 "samples_shaded": sum(s["samples"] for s in log),
                 "peak_sample_buffer_bytes": max(s["sample_buffer_bytes"] for s in log),
                 "rounds_per_chunk": [s["rounds"] for s in log], "rounds_total": sum(s["rounds"] for s in log),
                 "n_step_first_chunk": log[0]["n_steps"]}
        if "existing" in outs:
            for k in ("depth_lidar", "image_lidar"):
                a, b = outs[name][k].float(), outs["existing"][k].float()
                entry[f"max_dev_{k}_vs_existing"] = float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
            entry["frame_time_ratio_existing_over_alive"] = res["paths"]["existing"]["frame_ms_median"] / entry["frame_ms_median"]
        res["paths"][name] = entry
    # per-entry-point device time of one frame of each path (HIP events around every library call; a pass of its own)
    for name, kw in variants.items():
        _hip.enable_timers()
        render(**kw)
        torch.cuda.synchronize()
        tm = _hip.disable_timers()
        res["paths"][name]["entry_point_ms"] = {
            k: {"calls": len(v), "ms": round(sum(a.elapsed_time(b) for a, b, _ in v), 3)} for k, v in sorted(tm.items())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
