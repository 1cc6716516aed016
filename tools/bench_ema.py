#!/usr/bin/env python3
"""HIP-event times of the parameter average (csrc/ema.hip, nerf/ema.py) on the field of BASELINE config 1 — the
13.7 M-parameter hash table plus its MLP matrices — each against the torch-op formulation of torch_ema MEASURED IN THE
SAME RUN, the two sides alternating window by window:

    (a) lnh_ema_update                     vs  tmp = s - p; tmp.mul_(1 - decay); s.sub_(tmp) per parameter
    (b) lnh_ema_swap x 2                   vs  store() + copy_to() + restore() as torch ops, plus ONE re-cast of the table
                                               (fused.table16_of(training=False) pays one per render call)
    (c) staged full-frame evaluation (66 x 1030 rays, 4096 per chunk) inside LidarTrainer.ema_weights()
                                           vs  the same evaluation with the averaged weights copied in through `.data`
    (d) the captured training step (4096 rays) with ema_interval=1 vs without

    python tools/bench_ema.py [--rounds 5] [--reps 40] [--out profiles/ema_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps):
    """ms per call: HIP events around `reps` back-to-back calls on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(sides, rounds, reps, warm=3):
    """{name: [ms per call, one figure per round]}: every side warmed up, then `rounds` windows of each, alternating."""
    for fn in sides.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(timed(fn, reps))
    return out


def line(name, ms, traffic_mb=None):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    s = f"  {name:<58s} {med * 1e3:9.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}, {len(ms)} windows)"
    if traffic_mb:
        s += f"   {traffic_mb / med / 1e3:.2f} TB/s over {traffic_mb:.0f} MB"
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_ema.py: no GPU — these are device times, there is nothing to measure without one")
    import bench
    from lidarnerf import _hip
    from lidarnerf.nerf import fused
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=True, ema_decay=0.95,
                      render_kwargs=dict(num_steps=bench.NUM_STEPS, upsample_steps=bench.UPSAMPLE))
    poses = bench.synthetic_frames(60, dev)
    batches = [bench.make_batch(poses, s, 4096, 0, dev, (1, 1), "analytic") for s in range(8)]
    for s in range(24):  # a field that has moved, shadows that differ from it
        tr.step(*batches[s % 8])
        if s % 4 == 3:
            tr.ema_update()
    torch.cuda.synchronize()
    ema, tp = tr.ema, tr.table
    params, shadows = list(model.parameters()), tr.ema.shadow_params
    n_all = sum(p.numel() for p in params)
    mb = n_all * 4 / 1e6
    rows = [f"parameter average on {torch.cuda.get_device_name(0)}: {len(params)} tensors, {n_all} parameters "
            f"({tp.numel()} in the table), library {bench.lib_sha16()}",
            f"HIP events around {a.reps} back-to-back calls per window, {a.rounds} windows per side, sides alternating; "
            "median of the windows"]

    # ---- (a) the update
    w = 1.0 - 0.95

    def torch_update():
        for s, p in zip(shadows, params):
            tmp = s - p.detach()
            tmp.mul_(w)
            s.sub_(tmp)

    table, small, rest = ema._plan(params)
    assert table is not None and not rest, (table, small, rest)
    with torch.no_grad():
        t = alternate({"hip": lambda: ema._launch("lnh_ema_update", params, table, small, (w,)), "torch": torch_update},
                      a.rounds, a.reps)
    rows += ["", "(a) one averaging step over all parameters",
             line("lnh_ema_update (one launch)", t["hip"], 3 * mb),
             line(f"torch ops, 3 per tensor ({3 * len(params)} launches)", t["torch"], 8 * mb),
             f"  ratio torch / hip: {statistics.median(t['torch']) / statistics.median(t['hip']):.2f}"]

    # ---- (b) swap in and out
    def hip_swaps():
        ema.swap()
        ema.swap()

    def torch_store_copy_restore():
        kept = [p.detach().clone() for p in params]
        for s, p in zip(shadows, params):
            p.data.copy_(s)
        tp.detach().to(torch.half).contiguous()  # what table16_of(training=False) does on every render call
        for c, p in zip(kept, params):
            p.data.copy_(c)

    def recast():
        tp.detach().to(torch.half).contiguous()

    with torch.no_grad():
        t = alternate({"hip": hip_swaps, "torch": torch_store_copy_restore, "recast": recast}, a.rounds, a.reps)
    rows += ["", "(b) averaged weights in and out again",
             line("lnh_ema_swap x 2 (fp16 copy rewritten both times)", t["hip"], 2 * 4.5 * mb),
             line("torch: store + copy_to + restore + one re-cast", t["torch"], (3 * 2 + 1.5) * mb),
             line("  of which the re-cast (paid per render call)", t["recast"], 1.5 * mb),
             f"  ratio torch / hip: {statistics.median(t['torch']) / statistics.median(t['hip']):.2f}"]

    # ---- (c) full-frame evaluation on the averaged weights
    frame = bench.make_batch(poses, 0, 66 * 1030, 0, dev)
    kw = dict(cal_lidar_color=True, staged=True, max_ray_batch=4096, perturb=False, num_steps=bench.NUM_STEPS,
              upsample_steps=bench.UPSAMPLE)
    model.eval()

    def eval_hip():
        with tr.ema_weights():
            return model.render(frame[0], frame[1], **kw)

    def eval_data():
        kept = [p.detach().clone() for p in params]
        for s, p in zip(shadows, params):
            p.data.copy_(s)
        try:
            return model.render(frame[0], frame[1], **kw)
        finally:
            for c, p in zip(kept, params):
                p.data.copy_(c)

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        o1, o2 = eval_hip(), eval_data()
        same = all(torch.equal(o1[k], o2[k]) for k in ("depth_lidar", "image_lidar"))
        t = alternate({"hip": eval_hip, "data": eval_data}, a.rounds, max(a.reps // 8, 3), warm=2)
    model.train()
    calls = -(-66 * 1030 // 4096)
    rows += ["", f"(c) staged full-frame evaluation, 66 x 1030 rays in {calls} chunks of 4096 (both sides render the same bits: {same})",
             line("inside ema_weights() (2 swaps, persistent fp16 table)", t["hip"]),
             line(f"weights copied in through .data ({calls} re-casts of the table)", t["data"]),
             f"  ratio .data / ema_weights: {statistics.median(t['data']) / statistics.median(t['hip']):.3f}"]

    # ---- (d) the training step with and without an update per step
    state = {"i": 0}

    def step():
        tr.step(*batches[state["i"] % 8])
        state["i"] += 1

    def step_plain():
        tr.ema_interval = None
        step()

    def step_ema():
        tr.ema_interval = 1
        step()

    t = alternate({"plain": step_plain, "ema": step_ema}, a.rounds, a.reps)
    tr.ema_interval = None
    d = statistics.median(t["ema"]) - statistics.median(t["plain"])
    rows += ["", f"(d) captured training step, 4096 rays (graph: {tr.graph}, captures: {len(tr.capture_ms)}, error: {tr.graph_error})",
             line("step()", t["plain"]), line("step() with ema_interval=1", t["ema"]),
             f"  difference: {d * 1e3:.1f} us per step ({100 * d / statistics.median(t['plain']):.1f} %); the reference's "
             "cadence is one update per epoch"]
    text = "\n".join(rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
