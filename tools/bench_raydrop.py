#!/usr/bin/env python3
"""Time of one training step of the ray-drop MLP (lidarnerf/raydrop.py, csrc/raydrop.hip) against the reference's formulation —
the same network as a stock nn.Linear chain with torch.optim.Adam on the GPU, the loop body of raydrop_train_pcgen.py:448-482
without its logging (no loss.item(): the baseline is not charged for the reference's per-step host read) — at the consumer's
4 x 128 and the training CLI's default 8 x 256, N_rand = 2048; and of one full-frame inference (66 x 1030 = 67 980 rows).

The sides alternate window by window IN ONE PROCESS; every window runs for at least --window seconds and ends in a synchronise
(with one after every ~20 ms of queued calls); median and range over --rounds windows.  Device activities and synchronising
runtime calls per step are counted with torch.profiler over 20 steps in a pass of their own, which also gives the time per
kernel of the fused path.  There is no other baseline: the parent commit has no such path.

    python tools/bench_raydrop.py [--rounds 7] [--window 0.3] [--out profiles/raydrop_bench.txt]

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N_RAND, FRAME_ROWS, TABLE_ROWS = 2048, 66 * 1030, 64 * 2048
SHAPES = ((4, 128), (8, 256))


def table(n, dev, seed):
    """n training rows: unit direction, depth in [0, 80] with a fifth exactly 0, intensity, target (the rule of G16's record)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, device=dev), dim=1)
    depth = torch.rand(n, generator=g, device=dev) * 80
    depth = torch.where(torch.rand(n, generator=g, device=dev) < 0.2, torch.zeros_like(depth), depth)
    inten = torch.rand(n, generator=g, device=dev) * (depth > 0)
    target = ((depth > 0) & (d[:, 2] < 0.2)).float()
    return torch.cat([d, depth[:, None], inten[:, None], target[:, None]], dim=1).contiguous()


class Stock(torch.nn.Module):
    """The reference's RayDrop from stock layers."""

    def __init__(self, D, W):
        super().__init__()
        self.linears = torch.nn.ModuleList([torch.nn.Linear(5, W)] + [torch.nn.Linear(W, W) for _ in range(D - 1)])
        self.output_linear = torch.nn.Linear(W, 1)

    def forward(self, x):
        for lin in self.linears:
            x = torch.relu(lin(x))
        return self.output_linear(x)


class StockLoop:
    """The loop body of the reference's train() on the GPU."""

    def __init__(self, model, rows, schedule):
        self.model, self.rows, self.schedule, self.cursor, self.k = model, rows, schedule, 0, 0
        self.opt = torch.optim.Adam(params=list(model.parameters()), lr=5e-4, betas=(0.9, 0.999))

    def step(self):
        batch = self.rows[self.cursor:self.cursor + N_RAND]
        self.cursor += N_RAND
        if self.cursor >= self.rows.shape[0]:
            self.rows = self.rows[torch.randperm(self.rows.shape[0], device=self.rows.device)]
            self.cursor = 0
        out = self.model(batch[:, :5])
        self.opt.zero_grad()
        loss = torch.mean((out - batch[:, 5].unsqueeze(1)) ** 2)
        loss.backward()
        self.opt.step()
        self.k += 1
        for g in self.opt.param_groups:
            g["lr"] = float(self.schedule[min(self.k, len(self.schedule) - 1)])
        return loss


def window(fn, seconds, batch):
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(batch):
            fn()
        n += batch
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6, n


def alternate(sides, args):
    print("timing: " + " | ".join(sides), flush=True)
    batch = {}
    for k, fn in sides.items():  # one synchronised call sizes the batch: about 20 ms of work between two synchronisations
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        batch[k] = max(1, min(1024, int(0.02 / max(time.perf_counter() - t0, 1e-6))))
        window(fn, 0.05, batch[k])
    times, counts = {k: [] for k in sides}, {}
    for r in range(args.rounds):
        for k, fn in sides.items():
            us, counts[k] = window(fn, args.window, batch[k])
            times[k].append(us)
        print(f"  round {r + 1} of {args.rounds}", flush=True)
    return times, counts


def report(times, counts, lines):
    for k, v in times.items():
        lines.append(f"  {k:<44s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; ~{counts[k]} calls per window)")


def verdict(times, fused, stock, lines, what):
    a, b = times[fused], times[stock]
    wins = sum(x < y for x, y in zip(a, b))
    lines.append(f"  {what}: fused faster in {wins} of {len(a)} windows; medians {statistics.median(b) / statistics.median(a):.2f} x apart"
                 + ("" if wins == len(a) else "  — NOT faster in every window"))


def activities(fn, steps, lines, label):
    """Device activities and synchronising runtime calls per call of fn, and the kernels of the fused path, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        events = prof.events()
        device = [e for e in events if str(e.device_type).endswith("CUDA")]
        syncs = [e for e in events if not str(e.device_type).endswith("CUDA") and
                 any(s in e.name for s in ("Synchronize", "hipMemcpy", "cudaMemcpy"))]
        lines.append(f"  {label}: {len(device) / steps:.1f} device activities and {max(len(syncs) - 1, 0) / steps:.2f} synchronising "
                     f"or copying runtime calls per step (over {steps} steps; the one synchronise that ends the pass is not counted)")
        mine = {}
        for e in device:
            found = re.search(r"k_raydrop_\w+(<[^>]*>)?", e.name)
            if found:
                short = found.group(0)
                mine.setdefault(short, []).append(e.device_time if hasattr(e, "device_time") else e.cuda_time)
        for name, t in sorted(mine.items()):
            lines.append(f"      {name:<40s} {len(t) / steps:.1f} per step, {statistics.mean(t):7.1f} us each")
    except Exception as e:  # (the timings stand without it)
        lines.append(f"  {label}: device activities NOT MEASURED ({type(e).__name__}: {e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_raydrop: no GPU — nothing is measured without one")
    from lidarnerf.raydrop import RayDropMLP, RayDropTrainer
    dev = torch.device("cuda", 0)
    rows = table(TABLE_ROWS, dev, 1)
    frame = table(FRAME_ROWS, dev, 2)[:, :5].contiguous()
    lines = [f"ray-drop MLP: one training step and one full-frame inference ({torch.cuda.get_device_name(0)})",
             f"N_rand = {N_RAND} of a table of {TABLE_ROWS} rows; fp32 on both sides; us per call, windows of >= {args.window} s "
             f"ending in a synchronise, alternating, median of {args.rounds} rounds"]
    for D, W in SHAPES:
        torch.manual_seed(0)
        model = RayDropMLP(D, W).to(dev)
        tr = RayDropTrainer(model, rows.clone(), N_rand=N_RAND, seed=0)
        stock = Stock(D, W).to(dev)
        stock.load_state_dict(model.state_dict())
        loop = StockLoop(stock, rows.clone(), tr.lr_schedule)
        # the two sides compute the same thing: one step from the same parameters on the same batch
        a, b = tr.step().clone(), loop.step().detach().reshape(1)
        got = torch.cat([p.detach().reshape(-1) for p in stock.parameters()])
        lines.append(f"D = {D}, W = {W} ({model.num_parameters} parameters): first step, loss fused {float(a):.6f} / stock {float(b):.6f}, "
                     f"largest parameter difference after it {float((got - model.flat).abs().max()):.3g}")
        times, counts = alternate({"fused step (3 launches)": tr.step, "stock nn.Linear chain + torch.optim.Adam": loop.step}, args)
        report(times, counts, lines)
        verdict(times, "fused step (3 launches)", "stock nn.Linear chain + torch.optim.Adam", lines, "training step")
        activities(tr.step, 20, lines, "fused")
        activities(loop.step, 20, lines, "stock")
        with torch.no_grad():
            stock.load_state_dict(model.state_dict())  # (the windows trained the two sides for different numbers of steps)
            diff = float((model(frame) - stock(frame)).abs().max())
            times, counts = alternate({"fused inference, 67980 rows": lambda: model(frame),
                                       "stock inference, 67980 rows": lambda: stock(frame)}, args)
        report(times, counts, lines)
        verdict(times, "fused inference, 67980 rows", "stock inference, 67980 rows", lines, f"inference (same parameters; outputs differ by at most {diff:.3g})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
