#!/usr/bin/env python3
"""Time of mesh ray casting (lidarnerf/raycast.py, csrc/raycast.hip) on the mesh tools/bench_mesh.py uses — the bench model
after --train-steps steps, marching cubes at resolution 256 with the threshold at the --quantile quantile of the volume — for
one 66 x 1030 LiDAR frame from a sensor pose of the benchmark's synthetic sequence:

  build           RaycastingScene(vertices, triangles) at the default grid: bounds, count, scan, fill and its two host reads
  cast            cast_rays of the frame at the default grid, at a sweep of grid resolutions (the sweep is what
                  DEFAULT_CELLS_PER_TRIANGLE in lidarnerf/raycast.py was chosen from) and at (1, 1, 1) = all triangles
  staged render   the NeRF's own staged render of the same frame, for scale

The sides alternate window by window IN ONE PROCESS; every window runs for at least --window seconds and ends in a
synchronise; median and range over --rounds windows.  The results of every grid are compared with those of the first before
anything is timed (they must be identical).  There is no Open3D on the machines this project is built on, so there is NO
baseline against Embree: the file says so.

    python tools/bench_raycast.py [--rounds 7] [--window 0.3] [--out profiles/raycast_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

R = 256
H, W = 66, 1030
K = (2.0, 26.9)
SWEEP = (16, 32, 64, 96, 128, 192, 256, 384)


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
        lines.append(f"  {k:<52s} {statistics.median(v):9.3f} ms   (min {min(v):.3f} ... max {max(v):.3f}; ~{counts[k]} calls per window)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--all-triangles-rays", type=int, default=4096,
                    help="rays of the frame cast at (1, 1, 1): every ray reads every triangle, the time is scaled to the frame")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_raycast: no GPU — nothing is measured without one")
    import bench
    from lidarnerf import raycast
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
    flat = u.flatten()
    threshold = float(flat.kthvalue(max(1, int(args.quantile * flat.numel())))[0])
    v, t = mesh.marching_cubes(u, threshold)
    world = mesh.to_world_device(v, model.aabb_infer, R)
    del u, flat
    scene = raycast.RaycastingScene(world, t)
    rays_o, rays_d = scene.lidar_rays(K, poses[0], H, W)
    want = scene.cast_rays(rays_o, rays_d)
    hits = int((want["primitive_ids"] >= 0).sum())
    lines = [f"mesh ray casting on the bench model's mesh after {args.train_steps} steps ({torch.cuda.get_device_name(0)})",
             f"mesh: resolution {R}, threshold {threshold:.6g} (the {args.quantile} quantile): V = {scene.V} vertices, T = {scene.T} triangles",
             f"rays: one {H} x {W} frame = {H * W} rays from pose 0 of the synthetic sequence, {hits} of them hit",
             f"default grid {scene.grid} ({raycast.DEFAULT_CELLS_PER_TRIANGLE} cells per triangle): {scene.entries} list entries",
             f"ms per call, windows of >= {args.window} s ending in a synchronise, alternating, median of {args.rounds} rounds"]
    scenes = {}
    for n in SWEEP:
        s = raycast.RaycastingScene(world, t, grid_resolution=n)
        got = s.cast_rays(rays_o, rays_d)
        for k in want:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (n, k)  # grid = all triangles
        scenes[n] = s
    sides = {"build (default grid, two host reads)": lambda: raycast.RaycastingScene(world, t),
             f"cast, default grid {scene.grid}": lambda: scene.cast_rays(rays_o, rays_d)}
    for n, s in scenes.items():
        sides[f"cast, grid {n}^3 ({s.entries} entries)"] = (lambda s=s: s.cast_rays(rays_o, rays_d))
    times, counts = alternate(sides, args)
    report(times, counts, lines)
    best = min((statistics.median(x), k) for k, x in times.items() if k.startswith("cast, grid"))
    lines.append(f"  fastest of the sweep: {best[1]} at {best[0]:.3f} ms")
    # (1, 1, 1): every ray against every triangle — a subset of the frame, scaled
    n_sub = min(args.all_triangles_rays, H * W)
    pick = torch.linspace(0, H * W - 1, n_sub, device=dev).long()
    so, sd = rays_o[pick].contiguous(), rays_d[pick].contiguous()
    one = raycast.RaycastingScene(world, t, grid_resolution=1)
    got = one.cast_rays(so, sd)
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k][pick].view(torch.int32)), ("(1, 1, 1)", k)
    times1, counts1 = alternate({f"cast, grid (1, 1, 1), {n_sub} of the frame's rays": lambda: one.cast_rays(so, sd)},
                                argparse.Namespace(rounds=min(args.rounds, 3), window=args.window))
    report(times1, counts1, lines)
    ms1 = statistics.median(next(iter(times1.values())))
    lines.append(f"  ... scaled to the {H * W} rays of the frame: {ms1 * H * W / n_sub:.1f} ms (NOT MEASURED as a whole frame)")

    def staged():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return model.render(rays_o[None], rays_d[None], cal_lidar_color=True, staged=True, perturb=False,
                                num_steps=bench.NUM_STEPS, upsample_steps=bench.UPSAMPLE)

    was_training = model.training
    model.eval()
    try:
        times2, counts2 = alternate({"staged NeRF render of the same frame (for scale)": staged}, args)
        report(times2, counts2, lines)
    except Exception as e:
        lines.append(f"  staged NeRF render of the same frame: NOT MEASURED ({type(e).__name__}: {e})")
    model.train(was_training)
    lines.append("  against Open3D / Embree (the reference's RaycastingScene.cast_rays): NOT MEASURED — open3d is not installed here; "
                 "no baseline is invented")
    lines.append("  index-then-vertex fetch against a per-entry copy of the triangle: NOT MEASURED — only the first is built")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
