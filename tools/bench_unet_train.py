#!/usr/bin/env python3
"""Time of the ray-drop U-Net's training-mode forward (lidarnerf/unet_train.py: train_forward — weight pack, raw convolution, batch
statistics, BatchNorm + ReLU per layer) on one 66 x 1030 frame at N = 1 against the same network from stock torch modules
in train() mode, channels_last, under torch.autocast(fp16), autograd recording what its backward would need (as train_forward keeps
z).  The method is tools/bench_unet.py's: the sides alternate window by window in one process, median and range over --rounds windows;
device activities counted with torch.profiler in a pass of their own; per-launch times of the five new entry points from HIP events.

train_backward is timed alone and has NO stock counterpart: it stops short of the 3 x 3 convolutions' weight gradient, which a stock
backward cannot leave out, so a ratio would compare different work.

Since the 3 x 3 weight gradient (csrc/unet_train_wgrad.hip) the full backward — train_backward(conv_weights=True), all 64 gradients —
has that counterpart: train_forward + full backward is timed against the stock modules' forward + backward() (same mode, static loss
scale folded into the cotangent, gradients set to None between steps), and every layer's weight gradient is timed alone for each
variant of the kernel (HIP events around the entry point, variants alternating, median of --rounds).

The whole training step — RayDropUNetTrainer.train_step (lidarnerf/unet_trainer.py), eager and captured — is timed against the stock
loop (whole_step below), with device activities, synchronising calls and per-launch times of the three kernels of csrc/unet_train_step.hip.

    python tools/bench_unet_train.py [--rounds 7] [--window 0.3] [--out profiles/unet_train_bench.txt]

The stock side's BatchNorm2d layers run torch's own batch-norm kernels (the MIOpen switch is off around them, and only them; the
convolutions stay on MIOpen): with it on, this torch hands a channels_last training-mode batch norm to MIOpen, and the first such
call ended the process with a segmentation fault on an MI355X under torch 2.10 / ROCm 7.0.  Progress is printed stage by stage.

No GPU, no numbers: the tool refuses to run without one."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench_unet as B  # noqa: E402

NEW = ("lnh_unet_pack_conv3x3", "lnh_unet_conv3x3_raw", "lnh_unet_bn_stats", "lnh_unet_bn_relu", "lnh_unet_bn_relu_backward")
STEP = ("lnh_unet_loss_grad", "lnh_unet_grad_sumsq", "lnh_unet_rmsprop_step")
COPY_TBS = 6.29  # TB/s this card's copy kernels reach (MI355X): the yardstick of the optimizer pass


def say(what):
    print(f"[bench_unet_train] {what}", flush=True)


def native_batch_norm(stock):
    """BatchNorm2d.forward of every layer of `stock` with the MIOpen switch off (see the module docstring)."""
    for m in stock.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            inner = m.forward

            def forward(x, inner=inner):
                with torch.backends.cudnn.flags(enabled=False):
                    return inner(x)
            m.forward = forward
    return stock


def per_launch(fn, lines, title, frames=10, names=NEW):
    from lidarnerf import _hip
    fn()
    torch.cuda.synchronize()
    _hip.enable_timers(list(names))
    for _ in range(frames):
        fn()
    torch.cuda.synchronize()
    t = _hip.disable_timers()
    lines.append(f"  {title}, us per call (HIP events around each entry point, mean of {frames} frames; calls per frame; sum per frame):")
    for name in names:
        ev = t.get(name, [])
        if not ev:
            continue
        per = len(ev) // frames
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1, _ in ev]
        by_call = [statistics.mean(us[i::per]) for i in range(per)]
        lines.append(f"      {name:<28s} {statistics.mean(us):8.1f}   x {per:2d}   = {sum(by_call):8.1f}   (per call: "
                     + " ".join(f"{v:.0f}" for v in by_call) + ")")


def wgrad_per_layer(state, lines, rounds):
    """us per call of conv3x3_backward_weight (both launches) for every layer and variant, on the operands the backward left behind."""
    from lidarnerf import _hip, unet_train as ut
    variants = (("16-bit gathers", _hip.UNET_WGRAD_GATHER), ("ds_read_b64_tr_b16", _hip.UNET_WGRAD_TR))
    ws = state["views"]["ws_cw"]
    lines.append(f"  conv3x3_backward_weight per layer, us (HIP events around the entry point, variants alternating, median of {rounds}):")
    lines.append(f"      {'layer':<34s} {'pixels':>7s} " + " ".join(f"{name:>20s}" for name, _ in variants))
    total = [0.0] * len(variants)
    for lay in state["layers"]:
        def run(variant):
            ut.conv3x3_backward_weight(lay["operand"][0], lay["dz"], ws, lay["dweight"], src1=lay["operand"][1], pool=lay["pool"],
                                       variant=variant)
        us = [[] for _ in variants]
        for r in range(rounds + 1):
            for i, (_, variant) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(variant)
                e1.record()
                torch.cuda.synchronize()
                if r:  # (the first round warms up)
                    us[i].append(e0.elapsed_time(e1) * 1e3)
        med = [statistics.median(v) for v in us]
        total = [a + b for a, b in zip(total, med)]
        shape = f"{'pool ' if lay['pool'] else ''}{lay['cin']} -> {lay['cout']}" + (" (cat)" if lay["operand"][1] is not None else "")
        lines.append(f"      L{lay['level']} {shape:<31s} {lay['dz'].numel() // lay['cout']:7d} " + " ".join(f"{m:20.1f}" for m in med))
    lines.append(f"      {'sum of the 18 layers':<34s} {'':>7s} " + " ".join(f"{m:20.1f}" for m in total))


def whole_step(net, stock, x, lines, args):
    """RayDropUNetTrainer.train_step, eager and captured, against the stock loop: the stock modules in train() mode, channels_last,
    fp16 autocast, the loss of lidarnerf.unet_train in torch ops, a static loss scale, clip_grad_norm_ and RMSprop(foreach=True), no
    .item() anywhere.  Both sides run with lr = 0: the same kernels and the same traffic, and thousands of timed steps on one
    random frame cannot drive either net into non-finite values (which the device side would answer with cheaper, skipped steps).
    The eager and the captured trainer share one net, hence one cached training state and one set of gradient buffers (each has its
    own optimizer state): harmless at lr = 0, where no parameter moves, and wrong for anything but timing.  The stock side unscales
    with a _foreach_mul_ pass of its own, which GradScaler.unscale_ would fuse with its inf check; the comparison does not hang on
    it (the stock forward + backward() alone take longer than the whole device step)."""
    from lidarnerf import unet_train as ut
    from lidarnerf.unet_trainer import RayDropUNetTrainer
    masks = ((x[:, 1] < 50) & (x[:, 0] > -0.5)).float()
    eager = RayDropUNetTrainer(net, lr=0.0, graph=False)
    captured = RayDropUNetTrainer(net, lr=0.0, graph=True)
    params = [p for p in stock.parameters()]
    opt = torch.optim.RMSprop(params, lr=0.0, weight_decay=1e-8, momentum=0.999, foreach=True)

    def stock_step():
        opt.zero_grad(set_to_none=True)
        loss = ut.raydrop_unet_loss(stock(x).float(), masks)
        (loss * 1024.0).backward()
        torch._foreach_mul_([p.grad for p in params], 1.0 / 1024.0)
        torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
        opt.step()
        return loss

    say("first whole steps")
    for _ in range(2):  # the second call of the captured trainer captures
        eager.train_step(x, masks)
        captured.train_step(x, masks)
    stock_step()
    torch.cuda.synchronize()
    say("timing whole steps")
    lines.append("whole training step (forward, loss, full backward, unscale, clip, RMSprop; lr = 0 on every side; static scale 1024):")
    sides = {"RayDropUNetTrainer.train_step, eager": lambda: eager.train_step(x, masks),
             "RayDropUNetTrainer.train_step, captured": lambda: captured.train_step(x, masks),
             "stock loop": stock_step}
    times, counts = B.alternate(sides, args)
    for k, v in times.items():
        lines.append(f"  {k:<44s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; ~{counts[k]} calls per window)")
    st = times["stock loop"]
    for k in list(sides)[:2]:
        wins = sum(p < q for p, q in zip(times[k], st))
        lines.append(f"  {k}: faster than the stock loop in {wins} of {len(st)} windows; medians "
                     f"{statistics.median(st) / statistics.median(times[k]):.2f} x apart (stock / device)")
    for k, fn in sides.items():
        B.activities(fn, 10, lines, k)
    per_launch(lambda: eager.train_step(x, masks), lines, "train_step", names=STEP)
    n = sum(p.numel() for p in params)
    ideal = 28 * n / (COPY_TBS * 1e12) * 1e6
    from lidarnerf import _hip
    _hip.enable_timers(["lnh_unet_rmsprop_step"])
    for _ in range(10):
        eager.train_step(x, masks)
    torch.cuda.synchronize()
    us = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1, _ in _hip.disable_timers()["lnh_unet_rmsprop_step"])
    lines.append(f"  rmsprop_step: 28 bytes x {n} parameters = {28 * n / 1e9:.3f} GB, {ideal:.0f} us at {COPY_TBS} TB/s; measured {us:.0f} us "
                 f"(median of 10) = {ideal / us:.2f} of that rate")
    steps = eager.steps, captured.steps
    lines.append(f"  steps taken / skipped: eager {steps[0]}, captured {steps[1]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_unet_train: no GPU — nothing is measured without one")
    from lidarnerf import unet_train as ut
    from lidarnerf.unet import RayDropUNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    stock = B.Stock().train()
    net = RayDropUNet()
    net.load_state_dict(stock.state_dict())
    net = net.to(dev)
    stock = native_batch_norm(stock.to(dev).to(memory_format=torch.channels_last)).prepare()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(1, 10, B.H, B.W, generator=g, device=dev) * 2 - 1
    x[:, 1] = (x[:, 1] + 1) * 40
    d = (torch.rand(1, 1, B.H, B.W, generator=g, device=dev) - 0.5) * 1024
    lines = [f"ray-drop U-Net training: one {B.H} x {B.W} frame, N = 1 ({torch.cuda.get_device_name(0)})",
             f"train_forward: live fp32 parameters packed on the device, raw convolution -> batch statistics -> BatchNorm + ReLU per layer; "
             f"stock: torch modules in train() mode, channels_last, fp16 autocast, autograd recording, BatchNorm on torch's own kernels; us per frame, windows of >= "
             f"{args.window} s ending in a synchronise, alternating, median of {args.rounds} rounds"]
    say("first train_forward")
    logits, state = ut.train_forward(net, x)
    torch.cuda.synchronize()
    say("first train_backward")
    ut.train_backward(net, state, d)
    torch.cuda.synchronize()
    say("first stock forward")
    ref = stock(x).detach().float()
    torch.cuda.synchronize()
    say("timing")
    lines.append(f"same parameters: logits differ by at most {float((logits - ref).abs().max()):.3g} (standard deviation "
                 f"of the logits {float(logits.std()):.3g})")
    sides = {"train_forward": lambda: ut.train_forward(net, x), "stock modules, train(), autocast": lambda: stock(x)}
    times, counts = B.alternate(sides, args)
    for k, v in times.items():
        lines.append(f"  {k:<44s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; ~{counts[k]} calls per window)")
    fa, st = times["train_forward"], times["stock modules, train(), autocast"]
    wins = sum(p < q for p, q in zip(fa, st))
    lines.append(f"  train_forward faster in {wins} of {len(fa)} windows; medians {statistics.median(st) / statistics.median(fa):.2f} x apart")
    times, counts = B.alternate({"train_backward (no 3 x 3 weight gradient)": lambda: ut.train_backward(net, state, d)}, args)
    for k, v in times.items():
        lines.append(f"  {k:<44s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; ~{counts[k]} calls per window)"
                     "   — alone: no fair stock counterpart without the weight gradient")
    say("device activities")
    B.activities(lambda: ut.train_forward(net, x), 10, lines, "train_forward")
    B.activities(lambda: stock(x), 10, lines, "stock")
    B.activities(lambda: ut.train_backward(net, state, d), 10, lines, "train_backward")
    say("per-launch times")
    per_launch(lambda: ut.train_forward(net, x), lines, "train_forward")
    per_launch(lambda: ut.train_backward(net, state, d), lines, "train_backward")
    say("full backward")
    ut.train_backward(net, state, d, conv_weights=True)
    torch.cuda.synchronize()
    params = [p for p in stock.parameters()]

    def stock_step():
        for p in params:
            p.grad = None
        out = stock(x)
        out.backward(d.to(out.dtype))

    def device_step():
        ut.train_backward(net, ut.train_forward(net, x)[1], d, conv_weights=True)

    lines.append("full backward (all 64 gradients; the stock side: forward + backward() of the same modules, no optimizer on either side):")
    times, counts = B.alternate({"train_backward, all 64 gradients": lambda: ut.train_backward(net, state, d, conv_weights=True),
                                 "train_forward + full train_backward": device_step,
                                 "stock forward + backward()": stock_step}, args)
    for k, v in times.items():
        lines.append(f"  {k:<44s} {statistics.median(v):9.1f} us   (min {min(v):.1f} ... max {max(v):.1f}; ~{counts[k]} calls per window)")
    fa, st = times["train_forward + full train_backward"], times["stock forward + backward()"]
    wins = sum(p < q for p, q in zip(fa, st))
    lines.append(f"  device forward + full backward faster in {wins} of {len(fa)} windows; medians "
                 f"{statistics.median(st) / statistics.median(fa):.2f} x apart (stock / device)")
    B.activities(lambda: ut.train_backward(net, state, d, conv_weights=True), 10, lines, "train_backward, all 64 gradients")
    B.activities(stock_step, 10, lines, "stock forward + backward()")
    say("weight gradient per layer")
    wgrad_per_layer(state, lines, args.rounds)
    say("whole step")
    whole_step(net, stock, x, lines, args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
