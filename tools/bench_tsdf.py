#!/usr/bin/env python3
"""Time of the TSDF fusion (lidarnerf/tsdf.py, csrc/tsdf.hip): lnh_tsdf_integrate over 60 frames of 66 x 1030 into a 256^3 and a
512^3 lattice, TSDFVolume.extract_mesh pass by pass, and the whole MeshNVS.fit.

The scene is a box room of 40 x 30 x 8 rendered in closed form on the device from 60 poses along a path through it, each turned
about the vertical axis.  The other side for integrate is the same integration written in torch ops — one frame at a time,
broadcast over the lattice, float32 with atan2 in float64 as the kernel takes it.  What the double-precision atan2 costs is
timed against a probe build of the same kernel with atan2f (--atan2f-lib; its pixels differ, it is no product path):

    LNH_VARIANT=atan2f LNH_VARIANT_FILES="tsdf.hip core.hip" \\
    LNH_EXTRA_FLAGS='-DLNH_PANO_ATAN2_F32 -DLNH_VARIANT_TAG="atan2f"' python lidar-nerf_amd/build.py

The sides alternate window by window IN ONE PROCESS; every window runs for at
least --window seconds, every call in it ends in a synchronise; median and range over --rounds windows.  A kernel call includes the two fills
that clear sum and count.  The figures to judge integrate by are
the voxel-frame rate and the bytes of one pass over sum + count (read and written once per call, whatever the number of frames).

    python tools/bench_tsdf.py [--rounds 7] [--window 0.3] [--atan2f-lib lidar-nerf_amd/lib/liblidarnerf_hip_atan2f.so]
                               [--out profiles/tsdf_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAMES, H, W, K = 60, 66, 1030, (2.0, 26.9)
ROOM_LO, ROOM_HI = (-20.0, -15.0, -1.7), (20.0, 15.0, 6.3)
HBM_BYTES_PER_S = 8e12  # bench.py: HBM_PEAK_GBS
PASSES = ("k_tsdf_finalize", "k_mc_count", "k_mc_scan", "k_mc_vertices", "k_mc_triangles", "k_mesh_vertex_observed", "k_mf_count",
          "k_mf_scan", "k_mf_vertices", "k_mf_triangles")


def window(fn, seconds):
    """ms per call over at least `seconds`.  Every call ends in a synchronise: a kernel call returns at once, and a loop that
    only watches the host clock would queue minutes of device work before its window closes."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()
        n += 1
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


def scene(dev):
    """(panos [F,H,W], intensities [F,H,W], poses [F,4,4]) of the room on the device."""
    i = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    j = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    beta = -(i - W / 2) / W * 2 * math.pi
    alpha = (K[0] - j / H * K[1]) / 180 * math.pi
    local = torch.stack([torch.cos(alpha) * torch.cos(beta), torch.cos(alpha) * torch.sin(beta), torch.sin(alpha) + 0 * beta], -1)
    lo, hi = torch.tensor(ROOM_LO, dtype=torch.float64, device=dev), torch.tensor(ROOM_HI, dtype=torch.float64, device=dev)
    panos, poses = [], []
    for f in range(FRAMES):
        u = f / (FRAMES - 1)
        yaw = 0.8 * math.sin(2 * math.pi * u)
        o = torch.tensor([-14.0 + 28.0 * u, 6.0 * math.sin(2 * math.pi * u), 0.0], dtype=torch.float64, device=dev)
        R = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]],
                         dtype=torch.float64, device=dev)
        d = local @ R.T
        t = torch.where(d > 0, (hi - o) / d, torch.where(d < 0, (lo - o) / d, torch.full_like(d, math.inf)))
        panos.append(t.min(-1).values.float())
        pose = torch.eye(4, dtype=torch.float64, device=dev)
        pose[:3, :3], pose[:3, 3] = R, o
        poses.append(pose.float())
    panos = torch.stack(panos)
    return panos, (0.5 + 0.01 * panos).contiguous(), torch.stack(poses)


def torch_integrate(vol, panos, w2l, max_depth):
    """lnh_tsdf_integrate in torch ops, one frame at a time over the whole lattice: float32, atan2 in float64."""
    nx, ny, nz = vol.dims
    dev = vol.sum.device
    ax = [torch.from_numpy(vol.lo[a:a + 1]).to(dev) + torch.arange(n, dtype=torch.float32, device=dev) * float(vol.step[a])
          for a, n in enumerate(vol.dims)]
    px, py, pz = ax[0].view(nx, 1, 1), ax[1].view(1, ny, 1), ax[2].view(1, 1, nz)
    pi_f = torch.tensor(math.pi, dtype=torch.float32, device=dev)
    down = float(np.float32((float(np.float32(K[1])) - float(np.float32(K[0]))) / 180.0 * math.pi))
    # (0-dim device tensors: torch divides by a Python scalar through its reciprocal, which is not the kernel's division)
    scalar = lambda x: torch.tensor(float(np.float32(x)), dtype=torch.float32, device=dev)
    col_step, row_step = scalar(2.0 * math.pi / W), scalar(float(np.float32(K[1])) / 180.0 * math.pi / H)
    trunc = scalar(vol.truncation)
    s, c = vol.sum, vol.count
    for f in range(panos.shape[0]):
        m = w2l[f].tolist()
        qx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
        qy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
        qz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
        rho2 = qx * qx + qy * qy
        r = torch.sqrt(rho2 + qz * qz)
        beta = pi_f - torch.atan2(qy.double(), qx.double()).float()
        alpha = torch.atan2(qz.double(), torch.sqrt(rho2).double()).float() + down
        cf = torch.round(beta / col_step)
        rf = torch.round(float(H) - alpha / row_step)
        cf = torch.where(cf == float(W), torch.zeros_like(cf), cf)
        ok = (r < max_depth) & (r > 0) & (rf >= 0) & (rf < float(H)) & (cf >= 0) & (cf < float(W))
        pix = torch.where(ok, rf * float(W) + cf, torch.zeros_like(cf)).long()
        d = panos[f].reshape(-1)[pix]
        sd = d - r
        ok = ok & (d > 0) & (d < math.inf) & ~(sd < -trunc)
        s = torch.where(ok, s + torch.clamp(sd / trunc, max=1.0), s)
        c = c + ok.to(torch.int32)
    return s, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--count-calls", type=int, default=4)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--atan2f-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tsdf: no GPU — nothing is measured without one")
    from lidarnerf import _hip, nvs, tsdf
    dev = torch.device("cuda", 0)
    panos, intensities, poses = scene(dev)
    w2l = torch.stack([nvs.inverse_pose(p)[:3].reshape(12) for p in poses]).contiguous()
    panos = panos.contiguous()
    box = (np.asarray(ROOM_LO) - 0.5, np.asarray(ROOM_HI) + 0.5)
    lines = [f"TSDF fusion of {FRAMES} frames of {H} x {W} of a {ROOM_HI[0] - ROOM_LO[0]:g} x {ROOM_HI[1] - ROOM_LO[1]:g} x "
             f"{ROOM_HI[2] - ROOM_LO[2]:g} room ({torch.cuda.get_device_name(0)})",
             f"ms per call, windows of >= {args.window} s, every call ending in a synchronise, alternating, median of {args.rounds} rounds"]
    t_start = time.perf_counter()
    probe = None
    if args.atan2f_lib:
        import ctypes
        probe = ctypes.CDLL(os.path.abspath(args.atan2f_lib))
        probe.lnh_tsdf_integrate.argtypes = _hip._SIGS["lnh_tsdf_integrate"] + [ctypes.c_void_p]
        probe.lnh_tsdf_integrate.restype = ctypes.c_int
        probe.lnh_last_error.restype = ctypes.c_char_p

    def emit():
        """Print what is new and rewrite the file: a run that is cut short leaves what it measured."""
        print("\n".join(lines[emit.done:]) + f"\n[{time.perf_counter() - t_start:.0f} s]", flush=True)
        emit.done = len(lines)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    emit.done = 0

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def integrate_section(R):
        vol = tsdf.TSDFVolume(box, resolution=R)

        def kernel(lib=None):
            # the entry point itself with the matrices inverted once (TSDFVolume.integrate inverts them per call, frame by frame)
            vol.sum.zero_(), vol.count.zero_()
            args_ = (panos.data_ptr(), w2l.data_ptr(), FRAMES, H, W, K[0], K[1], 80.0, tsdf._f3(vol.lo), tsdf._f3(vol.step), *vol.dims,
                     vol.truncation, vol.sum.data_ptr(), vol.count.data_ptr())
            if lib is None:
                _hip.call("lnh_tsdf_integrate", *args_)
            elif lib.lnh_tsdf_integrate(*args_, _hip.stream()) != 0:
                raise RuntimeError(lib.lnh_last_error().decode())

        def in_torch():
            return torch_integrate(vol, panos, w2l, 80.0)

        vol.sum.zero_(), vol.count.zero_()
        want_s, want_c = in_torch()
        kernel()
        same = bool(torch.equal(vol.count, want_c)) and bool(torch.equal(vol.sum.view(torch.int32), want_s.view(torch.int32)))
        differing = int((vol.count != want_c).sum()) + int((vol.sum.view(torch.int32) != want_s.view(torch.int32)).sum())
        del want_s, want_c
        n = R ** 3
        sides = {"lnh_tsdf_integrate": kernel, "torch ops, frame by frame": in_torch}
        if probe is not None:
            sides["probe build with atan2f (not the contract)"] = lambda: kernel(probe)
        first = [once(fn) for fn in sides.values()]
        lines.append(f"integrate into {R}^3 ({n * 8 / 1e6:.0f} MB of sum + count; {int((vol.count > 0).sum())} points observed); kernel and "
                     f"torch ops give {'the same bits' if same else f'DIFFERENT results ({differing} words)'}; one call each before the "
                     f"windows: {', '.join(f'{x:.1f}' for x in first)} ms")
        emit()
        times, counts = alternate(sides, args)
        kernel()  # (the volume holds the product kernel's result again)
        report(times, counts, lines)
        a, c =(statistics.median(times[k]) for k in list(sides)[:2])
        wins = sum(k < t for k, t in zip(times["lnh_tsdf_integrate"], times["torch ops, frame by frame"]))
        lines.append(f"  torch ops / kernel: {c / a:.1f} x (medians); the kernel is faster in {wins} of {args.rounds} windows")
        if probe is not None:
            b = statistics.median(times["probe build with atan2f (not the contract)"])
            lines.append(f"  the double-precision atan2 costs {a - b:.3f} ms of {a:.3f} ms ({100 * (a - b) / a:.0f} %): kernel / atan2f probe = {a / b:.2f} x")
        else:
            lines.append("  cost of the double-precision atan2: NOT MEASURED (no --atan2f-lib given)")
        lines.append(f"  {n * FRAMES / (a * 1e-3) / 1e9:.1f} G voxel-frames / s; one pass over sum + count (read and written: "
                     f"{n * 16 / 1e6:.0f} MB) takes {n * 16 / HBM_BYTES_PER_S * 1e3:.3f} ms at 8 TB/s = {100 * n * 16 / HBM_BYTES_PER_S / (a * 1e-3):.2f} % "
                     "of the call")
        emit()
        return vol

    R = args.resolutions[0]
    vol = integrate_section(R)
    v, t = vol.extract_mesh()
    lines.append(f"extract_mesh at {R}^3: V = {v.shape[0]} vertices, T = {t.shape[0]} triangles")
    frames = [{"pano": panos[f], "intensities": intensities[f], "lidar_pose": poses[f], "lidar_K": K, "lidar_H": H, "lidar_W": W}
              for f in range(FRAMES)]
    fit = lambda: nvs.MeshNVS.fit(frames, resolution=R, box=box)
    lines.append(f"  one call each before the windows: extract_mesh {once(vol.extract_mesh):.1f} ms, MeshNVS.fit {once(fit):.1f} ms")
    emit()
    times, counts = alternate({"extract_mesh (finalize, cubes, mask, filter)": vol.extract_mesh,
                               f"MeshNVS.fit, {FRAMES} frames, resolution {R}": fit}, args)
    report(times, counts, lines)
    emit()
    try:
        per = pass_times(vol.extract_mesh, args.count_calls)
        for name in PASSES:
            lines.append(f"  pass {name:<24s} {sum(x for k, x in per.items() if name in k):8.4f} ms of device time per call")
        rest = sum(x for k, x in per.items() if not any(name in k for name in PASSES))
        lines.append(f"  other device activities  {rest:8.4f} ms per call (torch.profiler, {args.count_calls} calls)")
    except Exception as e:  # (a runtime whose profiler does not see the device)
        lines.append(f"  per-pass times: NOT MEASURED ({type(e).__name__}: {e})")
    emit()
    del vol, v, t
    for R in args.resolutions[1:]:
        torch.cuda.empty_cache()
        integrate_section(R)


if __name__ == "__main__":
    main()
