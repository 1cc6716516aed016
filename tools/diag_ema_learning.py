#!/usr/bin/env python3
"""The control profiles/r06_learning_distribution.md asks for: held-out depth error of the RAW against the AVERAGED weights
(LidarTrainer(ema_decay=0.95), ema_update() once per epoch of 60 steps as the reference does, nerf/utils.py:1257-1258) on the
scene and recipe of tools/diag_learning.py — 4096 rays per step, the analytic scene, fp16 gradients behind the dynamic loss
scale — per seed and learning rate.  The average does not touch the training trajectory (tests/test_ema_gpu.py), so the raw
column is the run tools/diag_learning.py would have made.

    python tools/diag_ema_learning.py --patch 1x1 --lr 1e-2 --seeds 16 [--steps 800] [--at 420,780,800]

One JSON line per run, then a markdown row per checkpoint (min / median / max over the seeds)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

EPOCH = 60  # steps per epoch: the 60 poses of the synthetic trajectory, one batch each


def run(patch, steps, at, seed, lr, decay):
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(seed)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=lr, iters=30000, fp16=True, scale=bench.SCALE, ema_decay=decay,
                      render_kwargs=dict(num_steps=768, upsample_steps=64))
    poses = bench.synthetic_frames(60, dev)
    batches = [bench.make_batch(poses, s, 4096, 0, dev, patch, "analytic") for s in range(60)]
    held = bench.make_batch(poses, 30, 4096, 1, dev, (1, 1), "analytic")
    torch.manual_seed(seed)

    def depth_error_m():
        model.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out = model.render(held[0], held[1], cal_lidar_color=True, staged=False, perturb=False, num_steps=768,
                               upsample_steps=64)
        model.train()
        err = (out["depth_lidar"][0].float() - held[2][0, :, 2]).abs() / bench.SCALE
        return round(float(err.median()), 3)

    kw = {} if patch == (1, 1) else {"patch": patch}
    rows = []
    for s in range(steps):
        tr.step(*batches[s % 60], **kw)
        if (s + 1) % EPOCH == 0:
            tr.ema_update()
        if s + 1 in at:
            raw = depth_error_m()
            with tr.ema_weights():
                avg = depth_error_m()
            rows.append(dict(step=s + 1, raw=raw, ema=avg, updates=tr.ema.num_updates, scale=float(tr.loss_scale),
                             taken=tr.steps_taken()))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", default="1x1")
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--seed0", type=int, default=0)
    ap.add_argument("--steps", type=int, default=800)
    ap.add_argument("--at", default="420,780,800", help="steps at which both sets of weights are evaluated")
    ap.add_argument("--decay", type=float, default=0.95)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/diag_ema_learning.py: needs a GPU")
    patch = tuple(int(v) for v in a.patch.split("x"))
    at = sorted(int(v) for v in a.at.split(","))
    runs = []
    for seed in range(a.seed0, a.seed0 + a.seeds):
        rows = run(patch, a.steps, set(at), seed, a.lr, a.decay)
        runs.append(rows)
        print(json.dumps(dict(patch=a.patch, lr=a.lr, seed=seed, rows=rows)), flush=True)
    mmm = lambda v: f"{min(v):.2f} / {statistics.median(v):.2f} / {max(v):.2f}"
    for i, step in enumerate(at):
        raw, avg = [r[i]["raw"] for r in runs], [r[i]["ema"] for r in runs]
        better = sum(e < r for e, r in zip(avg, raw))
        print(f"| {a.lr:g} | {a.patch} | {a.seeds} | {step} | {runs[0][i]['updates']} | {mmm(raw)} | {mmm(avg)} | "
              f"{sum(r > 0.45 for r in raw)} | {sum(e > 0.45 for e in avg)} | {better} |", flush=True)


if __name__ == "__main__":
    main()
