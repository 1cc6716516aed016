#!/usr/bin/env python3
"""Time of lidarnerf.convert.lidar_to_pano_with_intensities_fpa (z-buffer, first-peak averaging: count / scan / scatter / resolve,
csrc/convert.hip) against this library's closest-point lidar_to_pano_with_intensities (one 64-bit atomic-min pass + resolve) — the
floor: it reads the same points and writes the same two images, and keeps one point per pixel instead of ten.

66 x 1030 image, intrinsics (2.0, 26.9), two clouds that live on the device:
    frame       100 000 points, uniform over the image (one sweep)
    aggregate   5 000 000 points, skewed towards the lowest rows and short ranges (a sequence's frames projected into one view:
                near-ground pixels receive hundreds of points)
The two functions alternate window by window IN ONE PROCESS; every window runs for at least --window seconds and ends in a
synchronise; median and range over --rounds windows.  The time of each pass comes from torch.profiler (device duration of
each kernel, by name) over --count-calls calls.  No ratio is fixed in advance: the file records what was measured.

    python tools/bench_convert_fpa.py [--rounds 7] [--window 0.3] [--out profiles/convert_fpa_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, K = 66, 1030, (2.0, 26.9)
PASSES = ("k_lnh_zero_words", "k_fpa_count", "k_fpa_scan", "k_fpa_scatter", "k_fpa_resolve")


def cloud(n, skew, dev, seed):
    """[n, 4] float32 points whose image coordinates are uniform (skew = 1) or crowd the lowest rows (skew > 1)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    v = torch.rand(n, generator=g, device=dev, dtype=torch.float64) ** (1.0 / skew)  # row / H: 1 = the lowest row
    d = 2.0 + 76.0 * torch.rand(n, generator=g, device=dev, dtype=torch.float64) ** skew
    beta = u * 2 * np.pi
    alpha = (H - (v * H - 0.5).clamp(0, H - 0.6)) * (K[1] / 180 * np.pi / H)
    az, el = np.pi - beta, alpha - (K[1] - K[0]) / 180 * np.pi
    xyz = torch.stack([d * torch.cos(el) * torch.cos(az), d * torch.cos(el) * torch.sin(az), d * torch.sin(el)], -1)
    inten = torch.rand(n, 1, generator=g, device=dev, dtype=torch.float64)
    return torch.cat([xyz, inten], -1).float().contiguous()


def window(fn, seconds):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            fn()
            n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, n


def pass_times(fn, calls):
    """ms of device time per call of every kernel the call launches, by kernel name."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            out[e.name] = out.get(e.name, 0.0) + e.time_range.elapsed_us() / 1e3 / calls
    return out


def measure(title, pts, args, lines):
    from lidarnerf import convert
    sides = {"closest point (lnh_lidar_to_pano)": lambda: convert.lidar_to_pano_with_intensities(pts, H, W, K),
             "fpa (lnh_lidar_to_pano_fpa)": lambda: convert.lidar_to_pano_with_intensities_fpa(pts, H, W, K)}
    pano, _ = sides["fpa (lnh_lidar_to_pano_fpa)"]()
    near, _ = sides["closest point (lnh_lidar_to_pano)"]()
    assert torch.equal(pano != 0, near != 0)  # the same pixels are hit
    for fn in sides.values():
        window(fn, 0.1)
    times, counts = {k: [] for k in sides}, {}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            ms, counts[k] = window(fn, args.window)
            times[k].append(ms)
    hit = int((near != 0).sum())
    lines.append(f"{title}: {pts.shape[0]} points, {hit} of {H * W} pixels hit; ms per call (outputs and workspace from torch's "
                 f"allocator included), windows of >= {args.window} s ending in a synchronise, alternating, {args.rounds} rounds")
    for k, v in times.items():
        lines.append(f"  {k:<36s} {statistics.median(v):8.4f} ms   (min {min(v):.4f}, max {max(v):.4f}; ~{counts[k]} calls per window)")
    a, b = (statistics.median(v) for v in times.values())
    lines.append(f"  fpa / closest point: {b / a:.2f} x (medians)")
    try:
        per = pass_times(sides["fpa (lnh_lidar_to_pano_fpa)"], args.count_calls)
        for name in PASSES:
            ms = sum(v for k, v in per.items() if name in k)
            lines.append(f"  pass {name:<18s} {ms:8.4f} ms of device time per call")
        rest = sum(v for k, v in per.items() if not any(name in k for name in PASSES))
        lines.append(f"  other device activities  {rest:8.4f} ms per call (torch.profiler, {args.count_calls} calls)")
    except Exception as e:  # (a runtime whose profiler does not see the device)
        lines.append(f"  per-pass times: NOT MEASURED ({type(e).__name__}: {e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--count-calls", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_convert_fpa: no GPU — nothing is measured without one")
    dev = torch.device("cuda", 0)
    lines = [f"range-image conversion, {H} x {W}, z_buffer_len 10 ({torch.cuda.get_device_name(0)})"]
    measure("frame", cloud(100_000, 1.0, dev, 0), args, lines)
    measure("aggregate", cloud(5_000_000, 3.0, dev, 1), args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
