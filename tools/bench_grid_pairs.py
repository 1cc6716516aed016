#!/usr/bin/env python3
"""Forward schedule of the hash-grid encoder, measured: which levels to pair, and the interleave block.

    python tools/bench_grid_pairs.py [--rays 4096] [--rounds 7] [--parent-lib PATH] [--out FILE]

On the benchmark's geometry (4096 rays x 832 ray-ordered samples = 3.41 M points, fp16 tables, 16 levels, base 16, finest
32768, 2^19 rows) it times with HIP events
  * every level alone (a one-level call on the level's table slice, as tools/bench_grid.py --per-level does);
  * every candidate pair (finest with coarsest, ...) as a two-level call, level-major against interleaved;
  * the whole forward and the step's two row-mapped calls (768 coarse + 64 importance samples per ray) for every
    (max_pairs, block) of the sweep, the configurations visited in turn `rounds` times (median, min, max - min).
--parent-lib: a second liblidarnerf_hip.so (the parent commit's build) loaded side by side and timed in the same rounds."""
import argparse
import ctypes as C
import hashlib
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lidar-nerf_amd"), os.path.join(ROOT, "tools")]
from bench_grid import lidar_points  # noqa: E402
from lidarnerf import _hip  # noqa: E402
from lidarnerf.gridencoder.grid import level_offsets  # noqa: E402

FWD, MAPPED = "lnh_grid_encode_forward", "lnh_grid_encode_forward_mapped_ex"


def load(path):
    lib = C.CDLL(path)
    for n in (FWD, MAPPED):
        getattr(lib, n).argtypes = _hip._SIGS[n] + [C.c_void_p]
        getattr(lib, n).restype = C.c_int
    return lib


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(ts):
    return f"median {np.median(ts):7.1f}  min {min(ts):7.1f}  spread {max(ts) - min(ts):6.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    new = _hip.lib()
    new_fn = load(_hip.lib_path())
    parent = load(a.parent_lib) if a.parent_lib else None
    T, T_cur, Lv = 832, 768, 16
    x = lidar_points(a.rays, T)
    B = x.shape[0]
    pls = np.exp2(np.log2(32768 / 16) / 15)
    S = float(np.log2(pls))
    off = torch.from_numpy(level_offsets(3, Lv, pls, 16, 19, False))
    tab = ((torch.rand(int(off[-1]), 2, device="cuda") - 0.5) * 2e-4).half()
    out = torch.empty(Lv, B, 2, dtype=torch.half, device="cuda")
    stream = _hip.stream()
    say(f"box {socket.gethostname()}  {torch.cuda.get_device_name(0)}  B = {B} points")
    say(f"library {sha(_hip.lib_path())}" + (f"  parent library {sha(a.parent_lib)}" if parent else ""))

    def check(rc):
        if rc:
            raise RuntimeError(f"forward failed ({rc})")

    def whole(lib):
        check(getattr(lib, FWD)(x.data_ptr(), tab.data_ptr(), off.data_ptr(), out.data_ptr(), B, 3, 2, Lv, S, 16, None, 0, 0, 0, 1,
                                stream))

    def mapped(lib):
        for b, t, so in ((a.rays * T_cur, T_cur, 0), (a.rays * (T - T_cur), T - T_cur, T_cur)):
            check(getattr(lib, MAPPED)(x.data_ptr(), tab.data_ptr(), off.data_ptr(), out.data_ptr(), b, t, T, so, B, 2, Lv, S, 16,
                                       0, 1, stream))

    def sub_call(levels):
        """A call on the table slices of `levels` (one or two) that reproduces their resolutions and classes."""
        sc = [float(np.exp2(l * S) * 16 - 1) for l in levels]
        h = int(round(sc[0] + 1))
        s2 = float(np.log2((sc[-1] + 1) / h)) if len(levels) == 2 else 0.0
        rows = [int(off[l + 1] - off[l]) for l in levels]
        sub = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32)
        t = torch.cat([tab[int(off[l]):int(off[l + 1])] for l in levels]).contiguous()
        return lambda: check(getattr(new_fn, FWD)(x.data_ptr(), t.data_ptr(), sub.data_ptr(), out.data_ptr(), B, 3, 2,
                                                  len(levels), s2, h, None, 0, 0, 0, 1, stream))

    try:
        # ---- every level alone, every candidate pair
        new.lnh_grid_forward_set_schedule(0, 0)
        alone = []
        for l in range(Lv):
            f = sub_call([l])
            f()
            alone.append(min(event_us(f) for _ in range(a.rounds)))
        say("\nlevel alone, us (min of %d): " % a.rounds + " ".join(f"{l}:{t:.1f}" for l, t in enumerate(alone)))
        say(f"sum of the levels {sum(alone):.1f} us")
        say("\npair (fine, coarse): level-major / interleaved at block 8, 32, 128 (us, min)   sum of the two alone")
        for p in range(Lv // 2):
            hi, lo = Lv - 1 - p, p
            f = sub_call([lo, hi])
            row = []
            for pairs, blk in ((0, 0), (1, 8), (1, 32), (1, 128)):
                new.lnh_grid_forward_set_schedule(pairs, blk)
                f()
                row.append(min(event_us(f) for _ in range(a.rounds)))
            say(f"  ({hi:2d},{lo:2d})  {row[0]:7.1f} / {row[1]:7.1f} {row[2]:7.1f} {row[3]:7.1f}     {alone[hi] + alone[lo]:7.1f}")

        # ---- whole forward, every configuration visited in turn
        AUTO = 0xFFFFFFFF  # the library's default schedule
        configs = ([(0, 32), (AUTO, 0)] + [(p, g) for g in (8, 32, 128) for p in (2, 4, 6, 8)] +
                   [(p, 32) for p in (1, 3, 5, 7)])
        for name, fn in (("whole forward (one call, 3.41 M points)", whole), ("the step's two row-mapped calls", mapped)):
            ts = {c: [] for c in configs}
            tp = []
            for c in configs:  # warm-up
                new.lnh_grid_forward_set_schedule(*c)
                fn(new_fn)
            for _ in range(a.rounds):
                if parent:
                    tp.append(event_us(lambda: fn(parent)))
                for c in configs:
                    new.lnh_grid_forward_set_schedule(*c)
                    ts[c].append(event_us(lambda: fn(new_fn)))
            say(f"\n{name}, us over {a.rounds} rounds")
            if parent:
                say(f"  parent library          {stats(tp)}")
            for c in configs:
                label = "library default   " if c[0] == AUTO else f"pairs {c[0]}  block {c[1]:3d}"
                say(f"  {label}      {stats(ts[c])}" + ("   (level-major)" if c[0] == 0 else ""))
    finally:
        new.lnh_grid_forward_set_schedule(0xFFFFFFFF, 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
