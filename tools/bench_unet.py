#!/usr/bin/env python3
"""Time of one forward of the ray-drop U-Net (lidarnerf/unet.py, csrc/unet.hip) on one 66 x 1030 frame against the reference's
formulation — the same network from stock torch modules (nn.Conv2d, nn.BatchNorm2d in eval mode, nn.ReLU, nn.MaxPool2d,
nn.ConvTranspose2d, F.pad, torch.cat), channels_last, under torch.autocast(fp16): what lidarnvs/unet.py runs with --amp, written
fresh here.

The sides alternate window by window IN ONE PROCESS; every window runs for at least --window seconds and ends in a synchronise
(with one after every ~20 ms of queued calls); median and range over --rounds windows.  Device activities and synchronising
runtime calls per frame are counted with torch.profiler in a pass of their own.  The per-launch table pairs each of the fused
path's 24 launches with the stock ops that do the same work (HIP events around each, mean over 10 frames, a pass of its own; the
stock side's events include the gaps between its ops).  There is no other baseline: the parent commit has no such path.

    python tools/bench_unet.py [--rounds 7] [--window 0.3] [--out profiles/unet_bench.txt]

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
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W = 66, 1030
CH = (64, 128, 256, 512, 1024)


def double_conv(cin, cout):
    m = nn.Module()
    m.double_conv = nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True),
                                  nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
    return m


class Stock(nn.Module):
    """UNet(10, 1, bilinear=False) from stock layers, with the reference's state-dict names; forward() is a list of 24 segments,
    one per launch of the fused path, so that each can be timed on its own."""

    def __init__(self):
        super().__init__()
        self.inc = double_conv(10, 64)
        for i in range(4):
            d = nn.Module()
            d.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), double_conv(CH[i], CH[i + 1]))
            setattr(self, f"down{i + 1}", d)
        for i in range(4):
            u = nn.Module()
            u.up = nn.ConvTranspose2d(CH[4 - i], CH[3 - i], 2, stride=2)
            u.conv = double_conv(CH[4 - i], CH[3 - i])
            setattr(self, f"up{i + 1}", u)
        self.outc = nn.Module()
        self.outc.conv = nn.Conv2d(64, 1, 1)

    def segments(self):
        """[(label, fn(state))]: state is a dict holding the running tensor `x` and the skips."""
        segs = [("input", lambda s: s.__setitem__("x", s["in"].contiguous(memory_format=torch.channels_last)))]

        def conv(seq, k, label, pre=None):
            def run(s):
                x = pre(s) if pre else s["x"]
                s["x"] = seq[k + 2](seq[k + 1](seq[k](x)))
            segs.append((label, run))

        def keep(l):
            segs.append((None, lambda s: s.__setitem__(f"skip{l}", s["x"])))

        conv(self.inc.double_conv, 0, "inc.0")
        conv(self.inc.double_conv, 3, "inc.3")
        keep(0)
        for i in range(1, 5):
            d = getattr(self, f"down{i}").maxpool_conv
            conv(d[1].double_conv, 0, f"down{i}.0 (+pool)", pre=lambda s, d=d: d[0](s["x"]))
            conv(d[1].double_conv, 3, f"down{i}.3")
            keep(i)
        for i in range(1, 5):
            u = getattr(self, f"up{i}")
            segs.append((f"up{i}.up", lambda s, u=u: s.__setitem__("x", u.up(s["x"]))))

            def cat(s, l=4 - i):
                x2, x1 = s[f"skip{l}"], s["x"]
                x1 = F.pad(x1, [0, x2.shape[3] - x1.shape[3], 0, x2.shape[2] - x1.shape[2]])
                return torch.cat([x2, x1], dim=1)
            conv(u.conv.double_conv, 0, f"up{i}.0 (+pad, cat)", pre=cat)
            conv(u.conv.double_conv, 3, f"up{i}.3")
        segs.append(("outc", lambda s: s.__setitem__("x", self.outc.conv(s["x"]))))
        return segs

    def forward(self, x, events=None):
        s = {"in": x}
        with torch.autocast("cuda", dtype=torch.float16):
            for label, fn in self._segs:
                if events is not None and label:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(s)
                    e1.record()
                    events.setdefault(label, []).append((e0, e1))
                else:
                    fn(s)
        return s["x"]

    def prepare(self):
        self._segs = self.segments()
        return self


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
    for k, fn in sides.items():
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


def activities(fn, steps, lines, label):
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
                     f"or copying runtime calls per frame (over {steps} frames; the one synchronise that ends the pass is not counted)")
    except Exception as e:  # (the timings stand without it)
        lines.append(f"  {label}: device activities NOT MEASURED ({type(e).__name__}: {e})")


def per_launch(net, stock, x, lines, frames=10):
    """HIP events around each launch of the fused path (lidarnerf._hip's timers) and around the stock ops of the same work."""
    from lidarnerf import _hip
    labels = [label for label, _ in stock._segs if label]
    _hip.enable_timers(["lnh_unet_input", "lnh_unet_conv3x3", "lnh_unet_upconv2x2", "lnh_unet_head"])
    for _ in range(frames):
        net(x)
    torch.cuda.synchronize()
    t = _hip.disable_timers()
    fused = {}
    convs = [lab for lab in labels if lab != "input" and lab != "outc" and not lab.endswith(".up")]
    ups = [lab for lab in labels if lab.endswith(".up")]
    for name, names in (("lnh_unet_input", ["input"]), ("lnh_unet_conv3x3", convs), ("lnh_unet_upconv2x2", ups), ("lnh_unet_head", ["outc"])):
        for i, (e0, e1, _) in enumerate(t[name]):
            fused.setdefault(names[i % len(names)], []).append(e0.elapsed_time(e1) * 1e3)
    events = {}
    for _ in range(frames):
        stock(x, events)
    torch.cuda.synchronize()
    lines.append(f"  per launch, us (mean of {frames} frames; HIP events; the stock side's include the gaps between its ops):")
    lines.append(f"      {'launch':<24s} {'fused':>9s} {'stock':>9s}")
    total = [0.0, 0.0]
    for lab in labels:
        a, b = statistics.mean(fused[lab]), statistics.mean(e0.elapsed_time(e1) * 1e3 for e0, e1 in events[lab])
        total[0] += a
        total[1] += b
        lines.append(f"      {lab:<24s} {a:9.1f} {b:9.1f}" + ("   <- fused slower" if a > b else ""))
    lines.append(f"      {'sum':<24s} {total[0]:9.1f} {total[1]:9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_unet: no GPU — nothing is measured without one")
    from lidarnerf.unet import RayDropUNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    stock = Stock().eval()
    with torch.no_grad():
        for m in stock.modules():  # statistics a trained net would have, not the identity
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2), m.running_var.uniform_(0.5, 1.5), m.weight.uniform_(0.8, 1.2), m.bias.uniform_(-0.2, 0.2)
    net = RayDropUNet()
    net.load_state_dict(stock.state_dict())
    net = net.to(dev)
    stock = stock.to(dev).to(memory_format=torch.channels_last).prepare()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(1, 10, H, W, generator=g, device=dev) * 2 - 1
    x[:, 1] = (x[:, 1] + 1) * 40  # depth in [0, 80]
    lines = [f"ray-drop U-Net: one forward of a {H} x {W} frame ({torch.cuda.get_device_name(0)})",
             f"fused: fp16 NHWC kernels, 24 launches; stock: torch modules, channels_last, fp16 autocast; us per frame, windows of >= "
             f"{args.window} s ending in a synchronise, alternating, median of {args.rounds} rounds"]
    with torch.no_grad():
        a, b = net(x).clone(), stock(x).float()
        lines.append(f"same parameters: logits differ by at most {float((a - b).abs().max()):.3g} (standard deviation of the logits "
                     f"{float(b.std()):.3g})")
        sides = {"fused forward (24 launches)": lambda: net(x), "stock modules, channels_last, autocast": lambda: stock(x)}
        times, counts = alternate(sides, args)
        for k, v in times.items():
            lines.append(f"  {k:<44s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; ~{counts[k]} calls per window)")
        fa, st = times["fused forward (24 launches)"], times["stock modules, channels_last, autocast"]
        wins = sum(p < q for p, q in zip(fa, st))
        lines.append(f"  fused faster in {wins} of {len(fa)} windows; medians {statistics.median(st) / statistics.median(fa):.2f} x apart"
                     + ("" if wins == len(fa) else "  — NOT faster in every window"))
        activities(lambda: net(x), 10, lines, "fused")
        activities(lambda: stock(x), 10, lines, "stock")
        per_launch(net, stock, x, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
