#!/usr/bin/env python3
"""Wall time, device activities and host synchronisations per frame of the evaluation epilogue on one 66 x 1030 frame, the
two ways alternating window by window IN ONE PROCESS:

    (a) torch + meters   the reference's eval_step masking and loss written in torch ops (utils.py:926-946), loss.item(),
                         then metrics.MAEMeter / RMSEMeter / DepthMeter .update() — what a user of the fast trainer had to do
    (b) fused            metrics.FrameEvaluator.update() per frame + ONE measure() per window (csrc/eval_frame.hip)

Every window runs for at least --window seconds and ends in a synchronise; both sides are warmed first.  Device activities
per frame (kernels + copies) come from torch.profiler over --count-frames frames, host synchronisations from
torch.cuda.set_sync_debug_mode("warn") over the same frames.  The last block times the staged render of the frame on the
bench model, so that the epilogue's share of a whole evaluation frame is visible.

    python tools/bench_eval_frame.py [--rounds 5] [--window 0.5] [--out profiles/eval_frame_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H, W = 66, 1030
ALPHA_D, ALPHA_R, ALPHA_I = 1000.0, 1.0, 10.0


def make_frame(seed, scale):
    g = torch.Generator().manual_seed(seed)
    raydrop = (torch.rand(H, W, generator=g) < 0.75).float()
    gt = torch.stack([raydrop, torch.rand(H, W, generator=g), scale * (2 + 76 * torch.rand(H, W, generator=g))], -1)
    image = torch.rand(H * W, 2, generator=g)
    depth = (gt[..., 2] * (1 + 0.05 * torch.randn(H, W, generator=g))).reshape(-1)
    return gt[None].cuda(), image[None].cuda(), depth[None].cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--count-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval_frame: no GPU — nothing is measured without one")
    import bench
    from lidarnerf import metrics
    scale = bench.SCALE
    frames = [make_frame(s, scale) for s in range(8)]
    mae, rmse, dm = metrics.MAEMeter(1.0), metrics.RMSEMeter(), metrics.DepthMeter(scale)
    ev = metrics.FrameEvaluator(H, W, scale, alphas=(ALPHA_D, ALPHA_R, ALPHA_I), max_frames=0)
    last = {}

    def torch_frame(k):
        images_lidar, image, depth = frames[k % len(frames)]
        gt_raydrop = images_lidar[:, :, :, 0]
        gt_intensity = images_lidar[:, :, :, 1] * gt_raydrop
        gt_depth = images_lidar[:, :, :, 2] * gt_raydrop
        pred = image.reshape(1, H, W, 2)
        pred_raydrop = pred[:, :, :, 0]
        raydrop_mask = torch.where(pred_raydrop > 0.5, 1, 0)
        pred_intensity, pred_depth = pred[:, :, :, 1], depth.reshape(1, H, W)
        if ALPHA_R > 0 and (not torch.all(raydrop_mask == 0)):
            pred_intensity, pred_depth = pred_intensity * raydrop_mask, pred_depth * raydrop_mask
        loss = (ALPHA_D * (pred_depth - gt_depth).abs().mean() + ALPHA_R * ((pred_raydrop - gt_raydrop) ** 2).mean()
                + ALPHA_I * ((pred_intensity - gt_intensity) ** 2).mean())
        last["loss"] = loss.item()
        mae.update(pred_intensity, gt_intensity), rmse.update(pred_intensity, gt_intensity), dm.update(pred_depth, gt_depth)

    def torch_window_end():
        last["a"] = (mae.measure(), rmse.measure(), dm.measure())
        mae.clear(), rmse.clear(), dm.clear()

    def fused_frame(k):
        images_lidar, image, depth = frames[k % len(frames)]
        ev.update(image, depth, images_lidar)

    def fused_window_end():
        last["b"] = ev.measure()
        ev.clear()

    sides = {"(a) torch masking + MAE / RMSE / Depth meters": (torch_frame, torch_window_end),
             "(b) FrameEvaluator.update + one measure() per window": (fused_frame, fused_window_end)}

    def window(frame, end, seconds):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                frame(n)
                n += 1
        end()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6, n

    lines = [f"evaluation epilogue of one {H} x {W} frame ({torch.cuda.get_device_name(0)}), us of wall time per frame;",
             f"windows of >= {args.window} s ending in a synchronise, the two sides alternating, {args.rounds} rounds"]
    for frame, end in sides.values():
        window(frame, end, 0.2)
    times = {k: [] for k in sides}
    counts = {k: 0 for k in sides}
    for _ in range(args.rounds):
        for k, (frame, end) in sides.items():
            us, n = window(frame, end, args.window)
            times[k].append(us)
            counts[k] = n
    for k, v in times.items():
        lines.append(f"  {k:<56s} {statistics.median(v):9.1f} us   (min {min(v):.1f}, max {max(v):.1f}; "
                     + ", ".join(f"{x:.1f}" for x in v) + f"; ~{counts[k]} frames per window)")
    a, b = last["a"], last["b"]
    lines.append(f"  same numbers: (a) mae {a[0]:.6f} rmse {a[1]:.6f} depth {a[2]}")
    lines.append(f"                (b) mae {b['mae']:.6f} rmse {b['rmse']:.6f} depth {b['depth']}")

    from torch.profiler import ProfilerActivity, profile
    lines.append(f"device activities (kernels + copies, torch.profiler) and host synchronisations "
                 f"(torch.cuda.set_sync_debug_mode) per frame, over {args.count_frames} frames + the window's end:")
    for k, (frame, end) in sides.items():
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for n in range(args.count_frames):
                frame(n)
            torch.cuda.synchronize()
        per_frame = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA) / args.count_frames
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            end()
            torch.cuda.synchronize()
        at_end = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                for n in range(args.count_frames):
                    frame(n)
                syncs = len(caught)
                end()
                syncs_end = len(caught) - syncs
            sync_text = f"{syncs / args.count_frames:.1f} synchronising calls / frame (+ {syncs_end} at the end)"
        except RuntimeError as e:  # (a runtime without the sync debug mode)
            sync_text = f"synchronising calls not measured ({e})"
        finally:
            torch.cuda.set_sync_debug_mode("default")
        lines.append(f"  {k:<56s} {per_frame:6.1f} activities / frame (+ {at_end} at the window's end), "
                     + sync_text)

    # the whole frame: staged render of 66 x 1030 rays on the bench model (fp16 autocast, eval mode), then the epilogue
    from lidarnerf.dataset.rays import get_lidar_rays
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev).eval()
    pose = bench.synthetic_frames(1, dev)
    rays = get_lidar_rays(pose, bench.INTRINSICS, H, W, -1)
    rays_o, rays_d = rays["rays_o"].contiguous(), rays["rays_d"].contiguous()
    render_ms = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.render(rays_o, rays_d, cal_lidar_color=True, staged=True, perturb=False,
                               num_steps=bench.NUM_STEPS, upsample_steps=bench.UPSAMPLE)
            torch.cuda.synchronize()
            if rep:
                render_ms.append((time.perf_counter() - t0) * 1e3)
    assert out["depth_lidar"].numel() == H * W
    r = statistics.median(render_ms)
    lines.append(f"staged render of the frame ({H * W} rays, {bench.NUM_STEPS}+{bench.UPSAMPLE} samples, untrained bench model): "
                 f"{r:.1f} ms (median of {len(render_ms)}); render + epilogue: (a) {r + statistics.median(list(times.values())[0]) / 1e3:.2f} ms, "
                 f"(b) {r + statistics.median(list(times.values())[1]) / 1e3:.2f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
