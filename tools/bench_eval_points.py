#!/usr/bin/env python3
"""Wall time, device activities and host synchronisations per frame of the points meter (chamfer distance + F-score of the
clouds back-projected from the predicted and the ground-truth range image) on one 66 x 1030 frame, the two ways alternating
window by window IN ONE PROCESS:

    (a) PointsMeter            metrics.PointsMeter.update() per frame (two pano_to_lidar with a boolean-mask index, two
                               lnh_chamfer_nn, torch reductions, two float() reads) + measure() per window
    (b) FramePointsEvaluator   metrics.FramePointsEvaluator.update() per frame + ONE measure() per window
                               (csrc/eval_points.hip)

Two cases: "noisy" — the frame of tests/test_metrics_gpu.py::test_meters_match_restatement (about 80 % of the pixels valid,
2 % depth noise) — and "all valid", every pixel a return on both sides (the worst case: 67 980 x 67 980 pairs per direction).
Every window runs for at least --window seconds and ends in a synchronise; both sides are warmed first.  Device activities per
frame (kernels + copies) come from torch.profiler over --count-frames frames, host synchronisations from
torch.cuda.set_sync_debug_mode("warn") over the same frames.  The last block times the nearest-neighbour kernels alone with
device events: two lnh_chamfer_nn launches against one lnh_eval_points_nn on the same clouds.

    python tools/bench_eval_points.py [--case noisy|all] [--rounds 5] [--window 0.5] [--out profiles/eval_points_bench.txt]

One case per process (--case), so that a caller can bound each with a time limit of its own; --out appends.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, K, SCALE = 66, 1030, (2.0, 26.9), 0.0107848535


def make_frame(case, seed):
    """(pred_depth [H, W], images_lidar [H, W, 3]) on the device, depths in scaled units."""
    rng = np.random.default_rng(seed)
    valid = np.ones((1, H, W), bool) if case == "all" else rng.uniform(size=(1, H, W)) > 0.2
    gt = (rng.uniform(2.0, 70.0, (1, H, W)) * valid).astype(np.float32)
    extra = 0.0 if case == "all" else (gt == 0) * (rng.uniform(size=gt.shape) > 0.97) * 5.0
    pred = (gt * rng.normal(1.0, 0.02, gt.shape) + extra).astype(np.float32)
    images = np.stack([valid[0].astype(np.float32), rng.uniform(size=(H, W)).astype(np.float32),
                       np.where(valid[0], gt[0], 30.0).astype(np.float32) * np.float32(SCALE)], -1)
    return torch.from_numpy(pred[0] * np.float32(SCALE)).cuda(), torch.from_numpy(images).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("noisy", "all"), default="noisy")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--count-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval_points: no GPU — nothing is measured without one")
    from lidarnerf import _hip, metrics
    frames = [make_frame(args.case, 9 + s) for s in range(4)]
    pm = metrics.PointsMeter(SCALE, K)
    ev = metrics.FramePointsEvaluator(H, W, SCALE, K, max_frames=0)
    last = {}

    def meter_frame(k):
        pred, images = frames[k % len(frames)]
        pm.update(pred[None], (images[..., 2] * images[..., 0])[None])   # (what nerf/evaluate.py hands over)

    def meter_window_end():
        last["a"] = pm.measure()
        pm.clear()

    def fused_frame(k):
        pred, images = frames[k % len(frames)]
        ev.update(pred, images)

    def fused_window_end():
        last["b"] = ev.measure()
        ev.clear()

    sides = {"(a) PointsMeter.update + measure() per window": (meter_frame, meter_window_end),
             "(b) FramePointsEvaluator.update + one measure() per window": (fused_frame, fused_window_end)}

    def window(frame, end, seconds):
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < seconds:
            for _ in range(4):
                frame(n)
                n += 1
        end()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6, n

    fused_frame(0)
    torch.cuda.synchronize()
    n_pred, n_gt = (int(c) for c in ev.counts[:2])
    ev.clear()
    lines = [f"points meter of one {H} x {W} frame, case '{args.case}': {n_pred} predicted and {n_gt} ground-truth points "
             f"({torch.cuda.get_device_name(0)}), us of wall time per frame;",
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
        lines.append(f"  {k:<60s} {statistics.median(v):9.1f} us   (min {min(v):.1f}, max {max(v):.1f}; "
                     + ", ".join(f"{x:.1f}" for x in v) + f"; ~{counts[k]} frames per window)")
    ta, tb = list(times.values())
    lines.append(f"  ratio of the medians (a) / (b): {statistics.median(ta) / statistics.median(tb):.2f}; (b) below (a) in every "
                 f"round: {all(b < a for a, b in zip(ta, tb))}")
    lines.append(f"  same numbers: (a) {last['a']}  (b) {last['b']}")

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
        lines.append(f"  {k:<60s} {per_frame:6.1f} activities / frame (+ {at_end} at the window's end), " + sync_text)

    # the nearest-neighbour kernels alone, on the clouds of frame 0, between device events
    fused_frame(0)
    torch.cuda.synchronize()
    a, b = ev.clouds[0, :n_pred, :3].contiguous(), ev.clouds[1, :n_gt, :3].contiguous()
    d = torch.empty((2, H * W), device="cuda")
    i = torch.empty((2, H * W), dtype=torch.int32, device="cuda")
    ws, ws_bytes = ev._ws.data_ptr(), ev._ws.numel() * 8

    def two_chamfer():
        _hip.call("lnh_chamfer_nn", a.data_ptr(), n_pred, b.data_ptr(), n_gt, d[0].data_ptr(), i[0].data_ptr())
        _hip.call("lnh_chamfer_nn", b.data_ptr(), n_gt, a.data_ptr(), n_pred, d[1].data_ptr(), i[1].data_ptr())

    def one_points_nn():
        _hip.call("lnh_eval_points_nn", ev.clouds[0].data_ptr(), ev.clouds[1].data_ptr(), ev.counts.data_ptr(), H * W, ws,
                  ws_bytes, ev.dist[0].data_ptr(), ev.idx[0].data_ptr(), ev.dist[1].data_ptr(), ev.idx[1].data_ptr())

    lines.append("nearest-neighbour search alone (both directions, device events, median of 9 after 2 warm-up calls):")
    kernel_us = []
    for name, fn in (("2 x lnh_chamfer_nn", two_chamfer), ("1 x lnh_eval_points_nn (search + resolve)", one_points_nn)):
        ts = []
        for rep in range(11):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ts.append(e0.elapsed_time(e1) * 1e3)
        kernel_us.append(statistics.median(ts))
        lines.append(f"  {name:<44s} {statistics.median(ts):9.1f} us   (min {min(ts):.1f}, max {max(ts):.1f})")
    lines.append(f"  ratio: {kernel_us[0] / kernel_us[1]:.2f}; same distances: "
                 f"{torch.equal(d[0, :n_pred], ev.dist[0, :n_pred]) and torch.equal(d[1, :n_gt], ev.dist[1, :n_gt])}, same indices: "
                 f"{torch.equal(i[0, :n_pred], ev.idx[0, :n_pred]) and torch.equal(i[1, :n_gt], ev.idx[1, :n_gt])}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
