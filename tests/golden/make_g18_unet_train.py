#!/usr/bin/env python3
"""G18 (first part): the loss and the validation score of the reference's U-Net training loop from the reference's own functions,
and the reference's own UNet(10, 1, bilinear=False) in train() mode on one hashed batch, on the CPU.

    python tests/golden/make_g18_unet_train.py <reference checkout>

lidarnvs/unet.py is loaded by path (dice_coeff, dice_loss).  Logits and masks come from the hash of tests/unet_ref.py
(unet_train_ref.loss_case), which the tests evaluate again; only the results are stored.

g18_unet_loss.npz, per case k of unet_train_ref.LOSS_CASES:
  `loss64_<k>`      BCEWithLogitsLoss()(logits, masks) + dice_loss(sigmoid(logits), masks, multiclass=False) in float64 — the lines of
                    raydrop_train_poisson.py for n_classes = 1
  `grad64_<k>`      its gradient with respect to the logits, float64 [N, H, W]
  `loss32_<k>`      the same loss evaluated in float32
  `dice_eval64_<k>` evaluate()'s score: dice_coeff((sigmoid(logits) > 0.5).float(), masks, reduce_batch_first=False)
  `dice_soft64_<k>` dice_coeff(sigmoid(logits), masks, reduce_batch_first=True)

g18_unet_train.npz, from the reference's UNet in train() mode with the hashed state dict of unet_ref.hash_state_dict on
unet_train_ref.g18_train_batch() (2 x 10 x 23 x 37), cotangent unet_train_ref.g18_train_cotangent():
  `logits64`        float64 logits [2, 1, 23, 37] of the module cast to double; `std`: their standard deviation
  `dev_amp16`       max-norm deviation from them of the reference's own float32 module under torch.autocast("cpu", fp16)
  `running_<name>`  the six running statistics of inc / down4 / up4's first BatchNorm after that one float64 call
  `grad_norm_<name>` the L2 norm of the float64 gradient of six parameters (first and last convolution, a BatchNorm weight and bias,
                    a transposed convolution, the head) after logits.backward(cotangent)
  `dev_backward`    asserted here to be below 1e-9: the largest relative L2 distance, over all 64 parameters, between the reference's
                    loss.backward() and unet_train_ref.unet_backward_from_state on the restatement's own forward state
(The 31 M gradient values themselves are not stored.)

g18_unet_block_<b>.npz and g18_unet_block_<b>_grads.npz, per block b of unet_train_ref.G18_BLOCKS — the reference's DoubleConv(10, 64),
Down(64, 128), Up(128, 64, False) with a skip one row and one column larger, OutConv(64, 1) in train() mode, N = 2, 17 x 19, hashed
weights of the whole net, inputs g18_block_inputs, cotangent g18_block_cotangent in +-1:
  `out64` float64 output; `dev_amp16_out`: max-norm deviation of the float32 module under torch.autocast("cpu", fp16)
  `running_<name>` the running statistics after the float64 call; `dinput_<i>` f32: the input gradients
  `dev_amp16_<name>`, `dev_amp16_dinput_<i>`: relative L2 deviation of the autocast run's gradients (asserted here: below 0.1)
  _grads file: `<name>` f32, the float64 parameter gradients rounded to float32
  The maker asserts unet_train_ref.block_train against all of it to 1e-9 before it rounds.

g18_unet_record.npz: the reference's UNet, float32, hashed weights, one fixed batch 2 x 32 x 48 (unet_train_ref.g18_record_batch), the
loss lines of raydrop_train_poisson.py, RMSprop(lr=1e-4, momentum=0.999, weight_decay=1e-8, foreach=True), clip_grad_norm_(1.0), 16
steps: `loss32` [16]; `loss_amp` [16]: the same under torch.autocast("cpu", fp16) with a static loss scale of 1024 (gradients divided
by it before the clip); `dev_loss`: the largest per-step gap between the two.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_train_ref as T  # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_unet", os.path.join(root, "lidarnvs", "unet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    bce = torch.nn.BCEWithLogitsLoss()
    out = {}
    for k in range(len(T.LOSS_CASES)):
        logits, masks = T.loss_case(k)
        x = logits.clone().requires_grad_(True)
        loss = bce(x, masks.double()) + ref.dice_loss(torch.sigmoid(x), masks.double(), multiclass=False)
        loss.backward()
        x32 = logits.float()
        out[f"loss64_{k}"] = loss.detach().numpy()
        out[f"grad64_{k}"] = x.grad.numpy()
        out[f"loss32_{k}"] = (bce(x32, masks.float()) + ref.dice_loss(torch.sigmoid(x32), masks.float(), multiclass=False)).numpy()
        hard = (torch.sigmoid(logits.double()) > 0.5).double()
        out[f"dice_eval64_{k}"] = ref.dice_coeff(hard, masks.double(), reduce_batch_first=False).numpy()
        out[f"dice_soft64_{k}"] = ref.dice_coeff(torch.sigmoid(logits.double()), masks.double(), reduce_batch_first=True).numpy()
        print(k, T.LOSS_CASES[k], loss.item(), float(out[f"dice_eval64_{k}"]))
    path = os.path.join(HERE, "g18_unet_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")

    import unet_ref as R
    sd = R.hash_state_dict()
    x, cot = T.g18_train_batch(), T.g18_train_cotangent()
    net = ref.UNet(10, 1, bilinear=False)
    net.load_state_dict(sd)
    net.double().train()
    logits = net(x.double())
    logits.backward(cot)
    rec = {"logits64": logits.detach().numpy(), "std": np.float64(logits.detach().std())}
    buffers, params = dict(net.named_buffers()), dict(net.named_parameters())
    for name in T.G18_RUNNING:
        rec[f"running_{name}"] = buffers[name].detach().numpy().copy()
    for name in T.G18_GRAD_NORMS:
        rec[f"grad_norm_{name}"] = np.float64(params[name].grad.norm())
    got, state = T.unet_train_forward(sd, x)
    assert float((got - logits.detach()).abs().max()) < 1e-9
    grads = T.unet_backward_from_state(sd, state, cot)
    dev = max(float((grads[k] - p.grad).norm() / p.grad.norm()) for k, p in params.items())
    assert set(grads) == set(params) and dev < 1e-9, dev
    rec["dev_backward"] = np.float64(dev)
    amp = ref.UNet(10, 1, bilinear=False)
    amp.load_state_dict(sd)
    amp.train()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
        rec["dev_amp16"] = np.float64((amp(x).double() - logits.detach()).abs().max())
    print("train-mode logits: std", float(rec["std"]), "autocast deviation", float(rec["dev_amp16"]), "backward deviation", dev)
    path = os.path.join(HERE, "g18_unet_train.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    blocks(ref, sd)
    record(ref, sd)


def sub_state(sd, prefix):
    return {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def blocks(ref, sd):
    make = {"double_conv": lambda: ref.DoubleConv(10, 64), "down": lambda: ref.Down(64, 128), "up": lambda: ref.Up(128, 64, False),
            "out_conv": lambda: ref.OutConv(64, 1)}
    for name, (prefix, _, _) in T.G18_BLOCKS.items():
        bsd = sub_state(sd, prefix)
        inputs = T.g18_block_inputs(name)
        m = make[name]()
        m.load_state_dict(bsd)
        m.double().train()
        xs = [x.double().requires_grad_(True) for x in inputs]
        out = m(*xs)
        cot = T.g18_block_cotangent(name, out.shape)
        out.backward(cot)
        mine, backward, running = T.block_train(name, bsd, inputs)
        assert float((mine - out.detach()).abs().max()) < 1e-9, name
        grads, dins = backward(cot)
        params, buffers = dict(m.named_parameters()), dict(m.named_buffers())
        assert set(grads) == set(params)
        for k, p in params.items():
            assert rel(grads[k], p.grad) < 1e-9, (name, k)
        for g, x in zip(dins, xs):
            assert rel(g, x.grad) < 1e-9, name
        for k, v in running.items():
            assert float((v - buffers[k]).abs().max()) < 1e-12, (name, k)
        a = make[name]()
        a.load_state_dict(bsd)
        a.train()
        xa = [x.clone().requires_grad_(True) for x in inputs]
        with torch.autocast("cpu", dtype=torch.float16):
            oa = a(*xa)
        oa.backward(cot.to(oa.dtype))
        rec = {"out64": out.detach().numpy(), "dev_amp16_out": np.float64((oa.detach().double() - out.detach()).abs().max())}
        worst = 0.0
        for k, p in a.named_parameters():
            rec[f"dev_amp16_{k}"] = np.float64(rel(p.grad, params[k].grad))
            worst = max(worst, float(rec[f"dev_amp16_{k}"]))
        for i, (x, xr) in enumerate(zip(xa, xs)):
            rec[f"dinput_{i}"] = xr.grad.float().numpy()
            rec[f"dev_amp16_dinput_{i}"] = np.float64(rel(x.grad, xr.grad))
            worst = max(worst, float(rec[f"dev_amp16_dinput_{i}"]))
        assert worst < 0.1, (name, worst)
        for k in running:
            rec[f"running_{k}"] = buffers[k].detach().numpy().copy()
        np.savez_compressed(os.path.join(HERE, f"g18_unet_block_{name}.npz"), **rec)
        np.savez_compressed(os.path.join(HERE, f"g18_unet_block_{name}_grads.npz"), **{k: p.grad.float().numpy() for k, p in params.items()})
        sizes = [os.path.getsize(os.path.join(HERE, f"g18_unet_block_{name}{t}.npz")) for t in ("", "_grads")]
        print(f"block {name}: out dev_amp16 {float(rec['dev_amp16_out']):.3e}, worst gradient deviation {worst:.4f}, files {sizes}")
        assert max(sizes) < 1 << 20


def record(ref, sd):
    import torch.nn.functional as F
    images, masks = T.g18_record_batch()
    bce = torch.nn.BCEWithLogitsLoss()
    out = {}
    for key, amp in (("loss32", False), ("loss_amp", True)):
        net = ref.UNet(10, 1, bilinear=False)
        net.load_state_dict(sd)
        net.train()
        opt = torch.optim.RMSprop(net.parameters(), lr=1e-4, momentum=0.999, weight_decay=1e-8, foreach=True)
        losses = []
        for step in range(T.G18_STEPS):
            with torch.autocast("cpu", dtype=torch.float16, enabled=amp):
                pred = net(images)
                loss = bce(pred.squeeze(1), masks)
                loss += ref.dice_loss(F.sigmoid(pred.squeeze(1)), masks, multiclass=False)
            opt.zero_grad(set_to_none=True)
            (loss * 1024.0 if amp else loss).backward()
            if amp:
                for p in net.parameters():
                    p.grad.div_(1024.0)
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
            opt.step()
            losses.append(float(loss.detach().float()))
            print(key, step, losses[-1], flush=True)
        out[key] = np.asarray(losses, np.float64)
    out["dev_loss"] = np.float64(np.abs(out["loss32"] - out["loss_amp"]).max())
    print("dev_loss", float(out["dev_loss"]))
    np.savez_compressed(os.path.join(HERE, "g18_unet_record.npz"), **out)


if __name__ == "__main__":
    main()
