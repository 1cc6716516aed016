#!/usr/bin/env python3
"""Time of the mesh export (lidarnerf/nerf/mesh.py, csrc/mesh.hip) on the bench model at resolution 256: density_volume alone,
each marching-cubes pass (count, scan, emit = vertices + triangles), and the whole LidarTrainer.save_mesh with its PLY file.

The other side for density_volume is the reference's own way of filling the volume (nerf/utils.py:139-166): the same
lattice and the same model.density calls, but every chunk copied to the host into a NumPy volume.  The two alternate window
by window IN ONE PROCESS; every window runs for at least --window seconds and ends in a synchronise; median and range over
--rounds windows.  The time of each pass comes from torch.profiler (device duration of each kernel, by name) over
--count-calls calls, and is set against the time the pass would take if the fp32 volume were read once at 8 TB/s.

There is no PyMCubes on the machines this project is built on, so there is NO baseline for the marching-cubes half: the
file records what was measured and says so.  The model is trained for --train-steps steps on the benchmark's analytic scene
and the threshold is the --quantile quantile of its own volume, so that the surface is neither empty nor everywhere.

    python tools/bench_mesh.py [--rounds 7] [--window 0.3] [--out profiles/mesh_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

R = 256
HBM_BYTES_PER_S = 8e12  # bench.py: HBM_PEAK_GBS
PASSES = ("k_mc_count", "k_mc_scan", "k_mc_vertices", "k_mc_triangles")
READS_VOLUME = {"k_mc_count", "k_mc_vertices", "k_mc_triangles"}


def window(fn, seconds):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, n


def alternate(sides, args):
    print("timing: " + " | ".join(sides), flush=True)
    for fn in sides.values():
        window(fn, 0.05)
    times, counts = {k: [] for k in sides}, {}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            ms, counts[k] = window(fn, args.window)
            times[k].append(ms)
    return times, counts


def report(times, counts, lines):
    for k, v in times.items():
        lines.append(f"  {k:<44s} {statistics.median(v):9.3f} ms   (min {min(v):.3f} ... max {max(v):.3f}; ~{counts[k]} calls per window)")


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


def host_volume(model, resolution, S=128):
    """The volume filled the reference's way: one device -> host copy per chunk into a NumPy array."""
    lo_hi = model.aabb_infer.cpu().tolist()
    axes = [torch.linspace(lo_hi[a], lo_hi[3 + a], resolution).split(S) for a in range(3)]
    u = np.zeros([resolution] * 3, dtype=np.float32)
    with torch.no_grad():
        for i, xs in enumerate(axes[0]):
            for j, ys in enumerate(axes[1]):
                for k, zs in enumerate(axes[2]):
                    pts = torch.stack(torch.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
                    with torch.autocast("cuda", dtype=torch.float16):
                        sigma = model.density(pts.cuda())["sigma"]
                    u[i * S:i * S + len(xs), j * S:j * S + len(ys), k * S:k * S + len(zs)] = \
                        sigma.reshape(len(xs), len(ys), len(zs)).cpu().numpy()
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--count-calls", type=int, default=4)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh: no GPU — nothing is measured without one")
    import bench
    from lidarnerf.nerf import mesh
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE,
                      render_kwargs=dict(num_steps=bench.NUM_STEPS, upsample_steps=bench.UPSAMPLE))
    poses = bench.synthetic_frames(60, dev)
    for s in range(args.train_steps):
        tr.step(*bench.make_batch(poses, s, 4096, 0, dev, (1, 1), "analytic"))
    u = mesh.density_volume(model, R)
    assert np.array_equal(host_volume(model, R), u.cpu().numpy())  # both sides fill the same volume
    flat = u.flatten()
    threshold = float(flat.kthvalue(max(1, int(args.quantile * flat.numel())))[0])
    v, t = mesh.marching_cubes(u, threshold)
    V, T = v.shape[0], t.shape[0]
    lines = [f"mesh export at resolution {R} on the bench model after {args.train_steps} steps ({torch.cuda.get_device_name(0)})",
             f"threshold {threshold:.6g} (the {args.quantile} quantile of the volume): V = {V} vertices, T = {T} triangles",
             f"ms per call, windows of >= {args.window} s ending in a synchronise, alternating, median of {args.rounds} rounds"]
    times, counts = alternate({"density_volume (volume stays on the device)": lambda: mesh.density_volume(model, R),
                               "reference's loop (.cpu().numpy() per chunk)": lambda: host_volume(model, R)}, args)
    report(times, counts, lines)
    a, b = (statistics.median(x) for x in times.values())
    lines.append(f"  reference's loop / density_volume: {b / a:.2f} x (medians)")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.ply")
        times, counts = alternate({"marching_cubes (count, host read, emit)": lambda: mesh.marching_cubes(u, threshold),
                                   "save_mesh (volume, cubes, float64 map, PLY)": lambda: tr.save_mesh(path, R, threshold)}, args)
        ply_mb = os.path.getsize(path) / 1e6
    report(times, counts, lines)
    lines.append(f"  (the PLY file: {ply_mb:.1f} MB; outputs and workspace come from torch's allocator in every call)")
    lines.append("  marching cubes against PyMCubes: NOT MEASURED — mcubes is not installed here; no baseline is invented")
    volume_bytes = 4 * R ** 3
    try:
        per = pass_times(lambda: mesh.marching_cubes(u, threshold), args.count_calls)
        for name in PASSES:
            ms = sum(x for k, x in per.items() if name in k)
            note = ""
            if name in READS_VOLUME and ms > 0:
                rate = volume_bytes / (ms * 1e-3)
                note = (f"   volume read once: {rate / 1e12:.2f} TB/s = {100 * rate / HBM_BYTES_PER_S:.0f} % of the 8 TB/s roofline "
                        f"({volume_bytes / HBM_BYTES_PER_S * 1e3:.4f} ms)")
            lines.append(f"  pass {name:<16s} {ms:8.4f} ms of device time per call{note}")
        rest = sum(x for k, x in per.items() if not any(name in k for name in PASSES))
        lines.append(f"  other device activities {rest:8.4f} ms per call (torch.profiler, {args.count_calls} calls)")
    except Exception as e:  # (a runtime whose profiler does not see the device)
        lines.append(f"  per-pass times: NOT MEASURED ({type(e).__name__}: {e})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
