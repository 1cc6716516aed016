#!/usr/bin/env python3
"""Time of the nearest-neighbour intensity lookup (lidarnerf/knn.py, csrc/knn.hip) for the hit points of one 66 x 1030 LiDAR
frame (67 980 queries in frame order: consecutive queries are neighbours in space) against two clouds — 100 000 points (one
frame) and 5 000 000 points (an aggregated sequence, skewed towards the lowest rows and short ranges like
tools/bench_convert_fpa.py's):

  build           PointCloudIndex(points) at the default grid: bounds, count, scan, fill and its one host read
  search          search_knn at k = 1, 5, 9 at the default grid, and at (1, 1, 1) = every point, the floor it is measured against
                  (on the large cloud a subset of the queries, scaled: every query reads every point)
  sweep           mean_of_neighbours at k = 5 over a sweep of points per cell (what DEFAULT_POINTS_PER_CELL in lidarnerf/knn.py
                  is chosen from)
  chamfer         for k = 1 on the small cloud, lnh_chamfer_nn (the package's brute-force 1-nearest pass) alternating with it
  predict_frame   MeshNVS.predict_frame on the mesh tools/bench_raycast.py uses, next to its ray cast alone

The sides alternate window by window IN ONE PROCESS; every window runs for at least --window seconds and ends in a
synchronise (with one after every ~20 ms of queued calls); median and range over --rounds windows.  The results of every grid
are compared with those of (1, 1, 1) before anything is timed (they must be identical).  The condition the default has to
meet: faster than (1, 1, 1) on both clouds in every window.  There is no Open3D on the machines this project is built on, so
there is NO baseline against KDTreeFlann.

    python tools/bench_knn.py [--rounds 7] [--window 0.3] [--out profiles/knn_bench.txt]

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

import torch  # noqa: E402

H, W, K = 66, 1030, (2.0, 26.9)
KS = (1, 5, 9)
SWEEP = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)


def directions(u, v):
    """Unit directions of image coordinates u (column / W) and v (row / H, 1 = the lowest row), tools/bench_convert_fpa.py's."""
    beta = u * 2 * math.pi
    alpha = (H - (v * H - 0.5).clamp(0, H - 0.6)) * (K[1] / 180 * math.pi / H)
    az, el = math.pi - beta, alpha - (K[1] - K[0]) / 180 * math.pi
    return torch.stack([torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)], -1)


def cloud(n, skew, dev, seed):
    """[n, 3] float32 points whose image coordinates are uniform (skew = 1) or crowd the lowest rows and short ranges."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    v = torch.rand(n, generator=g, device=dev, dtype=torch.float64) ** (1.0 / skew)
    d = 2.0 + 76.0 * torch.rand(n, generator=g, device=dev, dtype=torch.float64) ** skew
    return (directions(u, v) * d[:, None]).float().contiguous()


def frame_queries(dev):
    """One point per pixel of the frame in row-major order, at a range that varies smoothly over the image."""
    r = torch.arange(H, device=dev, dtype=torch.float64)[:, None].expand(H, W).reshape(-1)
    c = torch.arange(W, device=dev, dtype=torch.float64)[None, :].expand(H, W).reshape(-1)
    u, v = (c + 0.5) / W, (r + 0.5) / H
    d = 2.0 + 76.0 * (0.5 + 0.25 * torch.sin(u * 37.0) + 0.2 * torch.cos(v * 5.0 + u * 11.0)) ** 2
    return (directions(u, v) * d[:, None]).float().contiguous()


def window(fn, seconds, batch):
    """Calls of fn for at least `seconds`, `batch` of them between two synchronisations (the launches are asynchronous: without
    a bound the host would queue minutes of work behind a slow side), ending in a synchronise."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(batch):
            fn()
        n += batch
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, n


def alternate(sides, args):
    print("timing: " + " | ".join(sides), flush=True)
    batch = {}
    for k, fn in sides.items():  # one synchronised call sizes the batch: about 20 ms of work between two synchronisations
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        batch[k] = max(1, min(256, int(0.02 / max(time.perf_counter() - t0, 1e-6))))
        window(fn, 0.05, batch[k])
    times, counts = {k: [] for k in sides}, {}
    for r in range(args.rounds):
        for k, fn in sides.items():
            ms, counts[k] = window(fn, args.window, batch[k])
            times[k].append(ms)
        print(f"  round {r + 1} of {args.rounds}", flush=True)
    return times, counts


def report(times, counts, lines, scale=None):
    for k, v in times.items():
        s = scale.get(k, 1.0) if scale else 1.0
        note = f", x {s:.2f} = {statistics.median(v) * s:.3f} ms for the whole frame" if s != 1.0 else ""
        lines.append(f"  {k:<58s} {statistics.median(v):9.3f} ms   (min {min(v):.3f} ... max {max(v):.3f}; ~{counts[k]} calls per window{note})")


def same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def bench_cloud(name, points, queries, sub, args, lines):
    from lidarnerf import knn
    dev = points.device
    values = torch.rand(points.shape[0], device=dev)
    index = knn.PointCloudIndex(points)
    one = knn.PointCloudIndex(points, grid_resolution=1)
    Q = queries.shape[0]
    pick = torch.linspace(0, Q - 1, sub, device=dev).long() if sub < Q else None
    q1 = queries if pick is None else queries[pick].contiguous()
    lines.append(f"{name}: N = {index.N} points, box {index.bounds[0]} ... {index.bounds[1]}")
    lines.append(f"  default grid {index.grid} ({knn.DEFAULT_POINTS_PER_CELL} points per cell); {Q} queries" +
                 ("" if pick is None else f"; (1, 1, 1) on {sub} of them, scaled"))
    for k in KS:  # the grid never changes the answer
        want = one.search_knn(q1, k)
        got = index.search_knn(queries, k)
        assert same(got if pick is None else [g[pick] for g in got], want), (name, k)
    sides = {"build (default grid, one host read)": lambda: knn.PointCloudIndex(points)}
    scale = {}
    for k in KS:
        sides[f"search k = {k}, default grid"] = (lambda k=k: index.search_knn(queries, k))
        label = f"search k = {k}, grid (1, 1, 1)" + ("" if pick is None else f", {sub} queries")
        sides[label] = (lambda k=k: one.search_knn(q1, k))
        scale[label] = Q / q1.shape[0]
    times, counts = alternate(sides, args)
    report(times, counts, lines, scale)
    ok = True
    for k in KS:
        a = times[f"search k = {k}, default grid"]
        label = next(s for s in times if s.startswith(f"search k = {k}, grid (1, 1, 1)"))
        b = [x * scale[label] for x in times[label]]
        faster = all(x < y for x, y in zip(a, b))
        ok &= faster
        lines.append(f"  k = {k}: default grid faster than (1, 1, 1) in {sum(x < y for x, y in zip(a, b))} of {len(a)} windows; "
                     f"medians {statistics.median(b) / statistics.median(a):.1f} x apart")
    lines.append(f"  condition (the default grid faster than (1, 1, 1) in every window): {'MET' if ok else 'NOT MET'}")
    # the sweep of points per cell, mean_of_neighbours at k = 5
    want = index.mean_of_neighbours(queries, values, 5)
    sweep = {}
    keep = knn.DEFAULT_POINTS_PER_CELL
    for per_cell in SWEEP:
        knn.DEFAULT_POINTS_PER_CELL = per_cell
        try:
            s = knn.PointCloudIndex(points)
        finally:
            knn.DEFAULT_POINTS_PER_CELL = keep
        assert torch.equal(s.mean_of_neighbours(queries, values, 5).view(torch.int32), want.view(torch.int32)), per_cell
        sweep[f"mean k = 5, {per_cell:g} points per cell, grid {s.grid}"] = (lambda s=s: s.mean_of_neighbours(queries, values, 5))
    times, counts = alternate(sweep, args)
    report(times, counts, lines)
    best = min((statistics.median(x), k) for k, x in times.items())
    lines.append(f"  fastest of the sweep: {best[1]} at {best[0]:.3f} ms")
    return index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--all-points-queries", type=int, default=2048,
                    help="queries searched at (1, 1, 1) on the large cloud: every query reads every point, the time is scaled")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knn: no GPU — nothing is measured without one")
    from lidarnerf import _hip
    dev = torch.device("cuda", 0)
    queries = frame_queries(dev)
    lines = [f"nearest-neighbour intensity lookup ({torch.cuda.get_device_name(0)})",
             f"queries: the {H * W} points of one {H} x {W} frame in row-major order",
             f"ms per call, windows of >= {args.window} s ending in a synchronise, alternating, median of {args.rounds} rounds"]
    small = cloud(100_000, 1.0, dev, 1)
    index = bench_cloud("one frame", small, queries, H * W, args, lines)
    big = cloud(5_000_000, 3.0, dev, 2)
    bench_cloud("aggregated sequence (skewed)", big, queries, args.all_points_queries, args, lines)
    del big
    # k = 1 against the chamfer meter's brute-force pass, small cloud
    Q = queries.shape[0]
    dist, idx = torch.empty(Q, device=dev), torch.empty(Q, dtype=torch.int32, device=dev)

    def chamfer():
        _hip.call("lnh_chamfer_nn", queries.data_ptr(), Q, small.data_ptr(), small.shape[0], dist.data_ptr(), idx.data_ptr())

    chamfer()
    got = index.search_knn(queries, 1)
    differ = int((idx != got[0][:, 0]).sum())
    lines.append(f"k = 1 on the one-frame cloud against lnh_chamfer_nn ({differ} of {Q} indices differ: its arithmetic is its own)")
    times, counts = alternate({"lnh_chamfer_nn (brute force, 1-nearest)": chamfer,
                               "search k = 1, default grid": lambda: index.search_knn(queries, 1)}, args)
    report(times, counts, lines)
    # the whole predict_frame on the bench model's mesh
    try:
        import bench
        from lidarnerf import nvs, raycast
        from lidarnerf.nerf import mesh
        from lidarnerf.nerf.train_step import LidarTrainer
        model = bench.build_model(dev)
        tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE,
                          render_kwargs=dict(num_steps=bench.NUM_STEPS, upsample_steps=bench.UPSAMPLE))
        poses = bench.synthetic_frames(60, dev)
        for s in range(args.train_steps):
            tr.step(*bench.make_batch(poses, s, 4096, 0, dev, (1, 1), "analytic"))
        u = mesh.density_volume(model, 256)
        flat = u.flatten()
        threshold = float(flat.kthvalue(max(1, int(args.quantile * flat.numel())))[0])
        v, t = mesh.marching_cubes(u, threshold)
        world = mesh.to_world_device(v, model.aabb_infer, 256)
        del u, flat
        scene = raycast.RaycastingScene(world, t)
        g = torch.Generator(device=dev).manual_seed(3)
        near = world[torch.randint(0, world.shape[0], (100_000,), generator=g, device=dev)]
        near = near + torch.randn(near.shape, generator=g, device=dev) * 1e-3
        frame = nvs.MeshNVS(scene, near, torch.rand(100_000, generator=g, device=dev))
        pose = poses[0].to(dev)
        hits = int(scene.intersect_lidar(K, pose, H, W)["masks"].sum())
        lines.append(f"predict_frame on the bench model's mesh after {args.train_steps} steps (T = {scene.T} triangles, grid {scene.grid}), "
                     f"cloud of 100000 points near it (grid {frame.index.grid}), k = {frame.k}: {hits} of {H * W} rays hit")
        times, counts = alternate({"intersect_lidar alone (rays + cast + hit dict)": lambda: scene.intersect_lidar(K, pose, H, W),
                                   "predict_frame(compact=False): no host read": lambda: frame.predict_frame(K, pose, H, W, compact=False),
                                   "predict_frame (with the four clouds)": lambda: frame.predict_frame(K, pose, H, W)}, args)
        report(times, counts, lines)
    except Exception as e:  # (the lookup's own figures above stand without it)
        lines.append(f"predict_frame on the bench model's mesh: NOT MEASURED ({type(e).__name__}: {e})")
    lines.append("against Open3D's KDTreeFlann (the reference's search_knn_vector_3d loop): NOT MEASURED — open3d is not installed "
                 "here; no baseline is invented")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
