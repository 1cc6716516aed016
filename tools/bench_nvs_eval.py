#!/usr/bin/env python3
"""Wall time, device activities and host synchronisations per frame of the NVS baselines' meters (lidarnvs/eval.py's
eval_points_and_pano) on one 66 x 1030 frame, the two ways alternating window by window IN ONE PROCESS:

    (a) torch ops            the image metrics in torch — clamps, thresholds, rmse, mae, and the 1-D SSIM of the contract
                             (tests/nvs_eval_ref.py: fp64 window moments over unfold(0, 7, 1); torch has no 1-D SSIM) — kept on
                             the device, plus metrics.FramePointsEvaluator.update for the point metrics; one host copy per window
    (b) NVSFrameEvaluator    nvs_eval.NVSFrameEvaluator.update() per frame + ONE measure() per window (csrc/eval_nvs.hip and the
                             same points kernels)

Both sides run the same nearest-neighbour kernels, which dominate a frame; the last block times the image meters alone — the
torch ops against the three lnh_nvs_eval_* launches — in windows of back-to-back calls.  Every window runs for at least --window seconds and ends in a synchronise; both
sides are warmed first; the median of --rounds windows is reported with min and max.  Device activities per frame (kernels +
copies) come from torch.profiler over --count-frames frames, host synchronisations from torch.cuda.set_sync_debug_mode("warn").

    python tools/bench_nvs_eval.py [--rounds 7] [--window 0.5] [--out profiles/nvs_eval_bench.txt]

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

H, W, K = 66, 1030, (2.0, 26.9)


def make_frame(seed):
    """(gt_pano, pd_pano, gt_int, pd_int) [H, W] on the device: about 80 % of the pixels a return, 2 % depth noise."""
    rng = np.random.default_rng(seed)
    valid = rng.uniform(size=(H, W)) > 0.2
    gt = (rng.uniform(2.0, 70.0, (H, W)) * valid).astype(np.float32)
    pd = (gt * rng.normal(1.0, 0.02, gt.shape) * (rng.uniform(size=(H, W)) > 0.05)).astype(np.float32)
    gi = (rng.uniform(size=(H, W)) * valid).astype(np.float32)
    pi = (gi * rng.normal(1.0, 0.05, gi.shape) * (pd != 0)).astype(np.float32)
    return tuple(torch.from_numpy(a).cuda() for a in (gt, pd, gi, pi))


def torch_image_metrics(gt, pd, gi, pi, s=1.0):
    """[rmse, a1, a2, a3, ssim, mae] as a device tensor (fp64); nothing is read back."""
    G, P = gt.flatten().clamp(1e-3, 80), pd.flatten().clamp(1e-3, 80)
    th = torch.maximum(G / P, P / G)
    a = [(th < t).double().mean() for t in (1.25, 1.5625, 1.953125)]
    rmse = ((G - P) ** 2).double().mean().sqrt()
    mae = (gi * s - pi * s).abs().double().mean()
    R = (G.max() - G.min()).double()
    x, y = G.double().unfold(0, 7, 1), P.double().unfold(0, 7, 1)
    ux, uy, uxx, uyy, uxy = x.sum(1) / 7, y.sum(1) / 7, (x * x).sum(1) / 7, (y * y).sum(1) / 7, (x * y).sum(1) / 7
    norm = 7.0 / 6.0
    vx, vy, vxy = norm * (uxx - ux * ux), norm * (uyy - uy * uy), norm * (uxy - ux * uy)
    c1, c2 = (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)
    S = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return torch.stack([rmse, a[0], a[1], a[2], S.mean(), mae])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--count-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nvs_eval: no GPU — nothing is measured without one")
    from lidarnerf import _hip, metrics
    from lidarnerf.nvs_eval import NVSFrameEvaluator
    frames = [make_frame(9 + s) for s in range(4)]
    gt3 = []
    for gt, *_ in frames:
        g = torch.zeros((H, W, 3), device="cuda")
        g[..., 0], g[..., 2] = 1.0, gt
        gt3.append(g)
    pts = metrics.FramePointsEvaluator(H, W, 1.0, K, max_frames=0)
    ev = NVSFrameEvaluator(H, W, K, max_frames=0)
    acc = torch.zeros(6, dtype=torch.float64, device="cuda")
    last = {}

    def torch_frame(k):
        gt, pd, gi, pi = frames[k % len(frames)]
        acc.add_(torch_image_metrics(gt, pd, gi, pi))
        pts.update(pd, gt3[k % len(frames)])

    def torch_window_end():
        n = int(pts.rows()[0][_hip.PTS_SLOT_NAMES.index("frames")])
        last["a"] = np.concatenate([acc.cpu().numpy() / n, pts.measure()])
        acc.zero_()
        pts.clear()

    def fused_frame(k):
        gt, pd, gi, pi = frames[k % len(frames)]
        ev.update({"pano": gt, "intensities": gi}, {"pano": pd, "intensities": pi})

    def fused_window_end():
        m = ev.measure()
        last["b"] = np.array([m[key] for key in ("depth_rmse", "depth_a1", "depth_a2", "depth_a3", "depth_ssim", "intensity_mae",
                                                 "chamfer", "f_score")])
        ev.clear()

    sides = {"(a) torch ops + FramePointsEvaluator, read at the window end": (torch_frame, torch_window_end),
             "(b) NVSFrameEvaluator.update + one measure() per window": (fused_frame, fused_window_end)}

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

    lines = [f"NVS meters of one {H} x {W} frame ({torch.cuda.get_device_name(0)}), us of wall time per frame;",
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
        lines.append(f"  {k:<60s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; "
                     + ", ".join(f"{x:.1f}" for x in v) + f"; ~{counts[k]} frames per window)")
    ta, tb = list(times.values())
    lines.append(f"  ratio of the medians (a) / (b): {statistics.median(ta) / statistics.median(tb):.2f}; (b) below (a) in every "
                 f"round: {all(b < a for a, b in zip(ta, tb))}")
    lines.append(f"  same numbers (rmse a1 a2 a3 ssim mae chamfer f_score): (a) {last['a']}  (b) {last['b']}")

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

    # the image meters alone: the torch ops against the three launches
    gt, pd, gi, pi = frames[0]
    ws, ws_bytes = ev._ws.data_ptr(), ev._ws.numel() * 8

    def three_launches():
        _hip.call("lnh_nvs_eval_frame", gt.data_ptr(), pd.data_ptr(), gi.data_ptr(), pi.data_ptr(), None, H, W, 1.0, ws, ws_bytes)
        _hip.call("lnh_nvs_eval_ssim", gt.data_ptr(), pd.data_ptr(), None, H, W, ws, ws_bytes)
        _hip.call("lnh_nvs_eval_finalize", H, W, ws, ws_bytes, ev.points.state[1].data_ptr(), ev.state.data_ptr(), None, 0)

    # one call is some 10 us: too short for a pair of events, so these are windows of back-to-back calls like the ones above
    lines.append(f"image meters alone, us per call in windows of >= {args.window / 2} s of back-to-back calls ending in a "
                 f"synchronise, alternating, {args.rounds} rounds (host enqueue time included where it is the longer):")
    alone_sides = {"torch ops (clamps, thresholds, sums, 1-D SSIM)": lambda k: torch_image_metrics(gt, pd, gi, pi),
                   "lnh_nvs_eval_frame + _ssim + _finalize": lambda k: three_launches()}
    alone = {k: [] for k in alone_sides}
    calls = {k: 0 for k in alone_sides}
    for fn in alone_sides.values():
        window(fn, lambda: None, 0.1)
    for _ in range(args.rounds):
        for k, fn in alone_sides.items():
            us, n = window(fn, lambda: None, args.window / 2)
            alone[k].append(us)
            calls[k] = n
    for k, v in alone.items():
        lines.append(f"  {k:<52s} {statistics.median(v):9.2f} us   (min {min(v):.2f} ... max {max(v):.2f}; ~{calls[k]} calls per window)")
    ma, mb = (statistics.median(v) for v in alone.values())
    lines.append(f"  ratio of the medians: {ma / mb:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
