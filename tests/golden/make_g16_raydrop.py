#!/usr/bin/env python3
"""G16: the reference's ray-drop MLP and its training pieces (lidarnvs/raydrop_train_pcgen.py: RayDrop, run_network, img2mse,
l1loss, cosine_scheduler, with torch.optim.Adam) and get_direction (lidarnvs/lidarnvs_pcgen.py:236-248), on the CPU.

    python tests/golden/make_g16_raydrop.py <reference checkout>

Both modules are loaded by path.  Empty stub modules stand in for what they import and this machine lacks or what is not under
test (imageio; camtools, lidarnvs.loader, lidarnvs.lidarnvs_base): no function used here touches them.

Three files next to this script (one would pass the size limit of a committed file; the split is by content):
  g16_raydrop.npz        D = 4, W = 128, biases made non-zero, 256 rows (unit directions, depths in [0, 80] with a fifth exactly
                         0): `params` f32 [P] in torch's order, `rows` f32 [256,6]; `out64`, `loss64_mse`, `loss64_l1`, `grad64_mse`
                         (f64 [P]) from the reference module cast to double; `dev_out`, `dev_loss_*`, `dev_grad_*` [10]: per tensor
                         the max-norm deviation of the reference's own fp32 run from that; `mag_grad_*` [10]: per tensor the largest
                         float64 magnitude.  `lr_exp`, `lr_cos`, `lr_cos_short` f64 [30]: the learning rate the reference's loop runs
                         step k at (exponential default; cosine default of 500000 steps with 1000 of warm-up; cosine over 40 steps
                         with 10 of warm-up).  get_direction: `dir_small` f64 [6,16,3] and, for 66 x 1030, its factors
                         `dir_ca`, `dir_sa` [66], `dir_cb`, `dir_sb` [1030] — asserted here to reproduce the reference's float64
                         image bit for bit as outer products — with `dir_dev_small`, `dir_dev_large`: NumPy's fp32 deviation.
                         Learning record: `learn_rows` f32 [8192,6], `learn_heldout` f32 [2048,6], `learn_loss` / `learn_acc` [5].
  g16_raydrop_l1.npz     `grad64_l1` f64 [P]
  g16_raydrop_adam.npz   `batches` f32 [20,64,6]; `p64_1`, `p64_20` f64 [P] after 1 and 20 steps of torch.optim.Adam in float64
                         on the reference's exponential schedule; `dev_p_1`, `dev_p_20`: max |p32 - p64| / lr of the fp32 run
"""
import argparse
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
D, W, LR = 4, 128, 5e-4
K = (2.0, 26.9)


class _Float64Arange:
    """numpy, with arange's dtype forced to float64 (get_direction asks for float32 pixel indices)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def arange(*args, **kw):
        kw["dtype"] = np.float64
        return np.arange(*args, **kw)


def load_reference(root):
    sys.path.insert(0, root)
    for name, names in (("imageio", ()), ("camtools", ()), ("lidarnvs.loader", ("extract_dataset_frame",)),
                        ("lidarnvs.lidarnvs_base", ("LidarNVSBase",))):
        mod = types.ModuleType(name)
        for n in names:
            setattr(mod, n, object)
        sys.modules[name] = mod
    out = []
    for name in ("raydrop_train_pcgen", "lidarnvs_pcgen"):
        spec = importlib.util.spec_from_file_location("lidarnvs." + name, os.path.join(root, "lidarnvs", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["lidarnvs." + name] = mod
        spec.loader.exec_module(mod)
        out.append(mod)
    return out


def table(rng, n):
    """n rows: unit direction, depth in [0, 80] with a fifth exactly 0, intensity in [0, 1]; no target yet."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    depth = rng.uniform(0, 80, n)
    depth[rng.permutation(n)[:n // 5]] = 0.0
    inten = np.where(depth > 0, rng.uniform(0, 1, n), 0.0)
    return np.concatenate([d, depth[:, None], inten[:, None]], axis=1).astype(np.float32)


def flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


def lr_of_step(ref, k, cos, n_iters=500000, warmup=1000, lrate=LR, decay=500, coslrate=5e-4, cosmin=5e-5):
    """The rate step k of the reference's loop runs at: `lrate` for k = 0, else what the loop set after step k - 1 from
    global_step = k - 1 (raydrop_train_pcgen.py:475-482)."""
    if k == 0:
        return lrate
    if cos:
        return ref.cosine_scheduler(base_value=coslrate, final_value=cosmin, globel_step=n_iters, warmup_iters=warmup)[k - 1]
    return lrate * (0.1 ** ((k - 1) / (decay * 1000)))


def evaluate(ref, model, rows, loss_fn):
    ident = torch.nn.Identity()
    model.zero_grad()
    out = ref.run_network(rows[:, :5], model, ident, ident)
    loss = loss_fn(out, rows[:, 5].unsqueeze(1))
    loss.backward()
    return out.detach().numpy().reshape(-1), float(loss.detach()), [p.grad.clone() for p in model.parameters()]


def adam_run(ref, model, batches, steps):
    ident = torch.nn.Identity()
    opt = torch.optim.Adam(params=list(model.parameters()), lr=LR, betas=(0.9, 0.999))
    for k in range(steps):
        out = ref.run_network(batches[k][:, :5], model, ident, ident)
        opt.zero_grad()
        loss = ref.img2mse(out, batches[k][:, 5].unsqueeze(1))
        loss.backward()
        opt.step()
        for g in opt.param_groups:  # (the reference's lag: set after the step, from the count before its increment)
            g["lr"] = lr_of_step(ref, k + 1, False)
    return flat(model.parameters())


def learn(ref, rows, heldout, seed):
    """The reference's loop: 300 steps, N_rand 256, the default exponential schedule, np.random.shuffle first, torch.randperm at
    the epoch boundary."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    ident = torch.nn.Identity()
    model = ref.RayDrop(D=D, W=W, input_ch=5)
    opt = torch.optim.Adam(params=list(model.parameters()), lr=LR, betas=(0.9, 0.999))
    rays = rows.copy()
    np.random.shuffle(rays)
    rays = torch.Tensor(rays)
    i_batch, losses = 0, []
    for k in range(300):
        batch = rays[i_batch:i_batch + 256]
        i_batch += 256
        if i_batch >= rays.shape[0]:
            rays = rays[torch.randperm(rays.shape[0])]
            i_batch = 0
        out = ref.run_network(batch[:, :5], model, ident, ident)
        opt.zero_grad()
        loss = ref.img2mse(out, batch[:, 5].unsqueeze(1))
        loss.backward()
        opt.step()
        for g in opt.param_groups:
            g["lr"] = lr_of_step(ref, k + 1, False)
        losses.append(loss.item())
    with torch.no_grad():
        h = torch.Tensor(heldout)
        pred = ref.run_network(h[:, :5], model, ident, ident).reshape(-1) > 0.5
    return float(np.mean(losses[-50:])), float((pred == (h[:, 5] > 0.5)).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference project")
    a = ap.parse_args()
    ref, pcgen = load_reference(a.reference)
    rng = np.random.default_rng(16)
    out, out_l1, out_adam = {}, {}, {}

    # ---- the network: outputs, loss, gradients
    torch.manual_seed(16)
    model = ref.RayDrop(D=D, W=W, input_ch=5)
    with torch.no_grad():
        for lin in list(model.linears) + [model.output_linear]:
            lin.bias.copy_(torch.from_numpy(rng.normal(0, 0.5, lin.bias.shape).astype(np.float32)))
    rows = table(rng, 256)
    rows = np.concatenate([rows, (rng.uniform(size=(256, 1)) < 0.5).astype(np.float32)], axis=1)
    out["params"], out["rows"] = flat(model.parameters()).astype(np.float32), rows
    model64 = copy.deepcopy(model).double()
    t32, t64 = torch.from_numpy(rows), torch.from_numpy(rows).double()
    sizes = [p.numel() for p in model.parameters()]
    for name, fn in (("mse", ref.img2mse), ("l1", ref.l1loss)):
        o64, l64, g64 = evaluate(ref, model64, t64, fn)
        o32, l32, g32 = evaluate(ref, model, t32, fn)
        assert o64.dtype == np.float64 and g64[0].dtype == torch.float64 and g32[0].dtype == torch.float32
        out["out64"], out["dev_out"] = o64, np.abs(o32.astype(np.float64) - o64).max()
        out[f"loss64_{name}"], out[f"dev_loss_{name}"] = l64, abs(l32 - l64)
        (out if name == "mse" else out_l1)[f"grad64_{name}"] = flat(g64)
        out[f"dev_grad_{name}"] = np.array([(a32.double() - a64).abs().max().item() for a32, a64 in zip(g32, g64)])
        out[f"mag_grad_{name}"] = np.array([a64.abs().max().item() for a64 in g64])
        assert all(m > 0 for m in out[f"mag_grad_{name}"]), "a tensor without gradient"
    assert sum(sizes) == len(out["params"]) == 50433

    # ---- Adam: 1 and 20 steps on 20 fixed batches
    batches = np.stack([np.concatenate([table(rng, 64), (rng.uniform(size=(64, 1)) < 0.5).astype(np.float32)], axis=1)
                        for _ in range(20)])
    out_adam["batches"] = batches
    b32 = torch.from_numpy(batches)
    for steps in (1, 20):
        p64 = adam_run(ref, copy.deepcopy(model).double(), b32.double(), steps)
        p32 = adam_run(ref, copy.deepcopy(model), b32, steps)
        assert p64.dtype == np.float64 and p32.dtype == np.float32
        out_adam[f"p64_{steps}"] = p64
        out_adam[f"dev_p_{steps}"] = np.abs(p32.astype(np.float64) - p64).max() / LR
        print(f"Adam, {steps} steps: fp32 deviates by {out_adam[f'dev_p_{steps}']:.3g} lr")

    # ---- the learning-rate sequences
    out["lr_exp"] = np.array([lr_of_step(ref, k, False) for k in range(30)], dtype=np.float64)
    out["lr_cos"] = np.array([lr_of_step(ref, k, True) for k in range(30)], dtype=np.float64)
    out["lr_cos_short"] = np.array([lr_of_step(ref, k, True, n_iters=40, warmup=10) for k in range(30)], dtype=np.float64)

    # ---- get_direction
    numpy32 = pcgen.np
    for H, Wd, tag in ((6, 16, "small"), (66, 1030, "large")):
        img32 = pcgen.get_direction(H, Wd, K)
        pcgen.np = _Float64Arange()
        img64 = pcgen.get_direction(H, Wd, K)
        flat_row = pcgen.get_direction(H, Wd, (0.0, K[1]))[0]  # alpha = 0 in row 0: cos 1, sin 0
        pcgen.np = numpy32
        assert img32.dtype == np.float32 and img64.dtype == np.float64 and img64.shape == (H, Wd, 3)
        out[f"dir_dev_{tag}"] = np.abs(img32.astype(np.float64) - img64).max()
        ca, sa, cb, sb = img64[:, Wd // 2, 0], img64[:, 0, 2], flat_row[:, 0], flat_row[:, 1]  # (beta = 0 at column W / 2)
        rebuilt = np.stack([ca[:, None] * cb[None, :], ca[:, None] * sb[None, :], np.broadcast_to(sa[:, None], (H, Wd))], -1)
        assert np.array_equal(rebuilt, img64), "the factors do not reproduce the reference's float64 image"
        if tag == "small":
            out["dir_small"] = img64
        else:
            out["dir_ca"], out["dir_sa"], out["dir_cb"], out["dir_sb"] = ca, sa, cb, sb
        print(f"get_direction {H} x {Wd}: NumPy fp32 deviates by {out[f'dir_dev_{tag}']:.3g}")

    # ---- the learning record
    def with_target(t):
        return np.concatenate([t, ((t[:, 3] > 0) & (t[:, 2] < 0.2)).astype(np.float32)[:, None]], axis=1)
    learn_rows, heldout = with_target(table(rng, 8192)), with_target(table(rng, 2048))
    out["learn_rows"], out["learn_heldout"] = learn_rows, heldout
    record = [learn(ref, learn_rows, heldout, seed) for seed in range(5)]
    out["learn_loss"], out["learn_acc"] = np.array([r[0] for r in record]), np.array([r[1] for r in record])
    for seed, (loss, acc) in enumerate(record):
        print(f"learning, shuffle {seed}: mean loss of the last 50 steps {loss:.5f}, held-out accuracy {acc:.4f}")

    # ---- the NumPy restatement (tests/raydrop_ref.py) equals every float64 tensor to 1e-12 relative
    sys.path.insert(0, os.path.dirname(HERE))
    import raydrop_ref as rr
    for name, lt in (("mse", 0), ("l1", 1)):
        o, num, loss, grad = rr.loss_and_grad(out["params"].astype(np.float64), D, W, rows.astype(np.float64), lt)
        want = (out if name == "mse" else out_l1)[f"grad64_{name}"]
        assert np.abs(o - out["out64"]).max() <= 1e-12 * np.abs(out["out64"]).max()
        assert abs(loss - out[f"loss64_{name}"]) <= 1e-12 * abs(loss)
        assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max(), name

    for name, d in (("g16_raydrop", out), ("g16_raydrop_l1", out_l1), ("g16_raydrop_adam", out_adam)):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(f"wrote {path}: {size / 1024:.0f} KiB")
        assert size < (1 << 20), "a committed file must stay under 1 MiB"
    print("deviations of the reference's own fp32 run: out %.3g, loss mse %.3g l1 %.3g" %
          (out["dev_out"], out["dev_loss_mse"], out["dev_loss_l1"]))
    print("  grad mse", np.array2string(out["dev_grad_mse"], precision=3), "\n  grad l1 ", np.array2string(out["dev_grad_l1"], precision=3))


if __name__ == "__main__":
    main()
