#!/usr/bin/env python3
"""G17: the reference's ray-drop U-Net (lidarnvs/unet.py: UNet(10, 1, bilinear=False), DoubleConv, Down, Up, OutConv) in eval mode
on the CPU.

    python tests/golden/make_g17_unet.py <reference checkout>

lidarnvs/unet.py is loaded by path.  The net has 31 M parameters, so nothing of it is stored: every weight, BatchNorm statistic and
input comes from the integer hash of tests/unet_ref.py (hash_state_dict, g17_image, g17_block_inputs), which the tests evaluate again.

Files next to this script (split by content to stay under the size limit of a committed file):
  g17_unet.npz         `names` / `shapes`: the state dict of the reference's UNet(10, 1, False), in its order.  Per block b of
                       unet_ref.G17_BLOCKS (DoubleConv(10, 64), Down(64, 128), Up(128, 64, False) with a skip one row and one column
                       larger, OutConv(64, 1); inputs 17 x 19): `block_<b>` f64, the reference module cast to double, and
                       `dev_amp16_block_<b>`: the max-norm deviation from it of the reference's own float32 module under
                       torch.autocast("cpu", dtype=torch.float16).  `logits64_0` f64 [1, 1, 23, 37] and `dev_amp16_0` likewise for the
                       whole net; `dev_amp16_1` for 66 x 1030; `std_0`, `std_1`: the standard deviation of the float64 logits;
                       `left_out_0`, `left_out_1`: the share of pixels with |logit64| <= 2 dev_amp16 (asserted here: below 5 %, and
                       the reference's autocast mask equal to logit64 > 0 at every other pixel); `dev_quant_*`: the max-norm
                       distance of unet_ref's quantize=True restatement from float64, per block and per size.
  g17_unet_frame.npz   `logits64_1` f64 [1, 1, 66, 1030]
  g17_unet_quant.npz   `quant_0`, `quant_1` f32: the quantize=True restatement's logits (fp32 values by construction)
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_ref as R  # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_unet", os.path.join(root, "lidarnvs", "unet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sub_state(sd, prefix):
    return {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}


def run_both(module, inputs):
    """(float64 output of the module cast to double, max-norm deviation of its float32 self under fp16 autocast)."""
    module.eval()
    with torch.no_grad():
        want = module.double()(*[x.double() for x in inputs])
        module.float()
        with torch.autocast("cpu", dtype=torch.float16):
            amp = module(*inputs)
    return want, amp.double(), float((amp.double() - want).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    ref = load_reference(ap.parse_args().reference)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd = R.hash_state_dict()
    net = ref.UNet(10, 1, False)
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert spec == R.state_spec(10), "tests/unet_ref.py: state_spec differs from the reference's state dict"
    net.load_state_dict(sd)
    out = {"names": np.array([k for k, _ in spec]), "shapes": np.array([",".join(map(str, s)) for _, s in spec])}
    frame, quant = {}, {}

    blocks = {"double_conv": ref.DoubleConv(10, 64), "down": ref.Down(64, 128), "up": ref.Up(128, 64, False),
              "out_conv": ref.OutConv(64, 1)}
    for name, module in blocks.items():
        module.load_state_dict(sub_state(sd, R.G17_BLOCKS[name][0]))
        inputs = R.g17_block_inputs(name)
        want, _, dev = run_both(module, inputs)
        mine = R.block_forward(name, sd, inputs)
        assert float((mine - want).abs().max()) < 1e-10, name
        out[f"block_{name}"] = want.numpy()
        out[f"dev_amp16_block_{name}"] = dev
        out[f"dev_quant_block_{name}"] = float((R.block_forward(name, sd, inputs, quantize=True) - want).abs().max())
        print(f"block {name}: {tuple(want.shape)}  dev_amp16 {dev:.3e}  dev_quant {out[f'dev_quant_block_{name}']:.3e}")

    for i, (H, W) in enumerate(R.G17_SIZES):
        x = R.g17_image(i)
        want, amp, dev = run_both(net, [x])
        mine = R.unet_forward(sd, x)
        assert float((mine - want).abs().max()) < 1e-10
        q = R.unet_forward(sd, x, quantize=True)
        sure = want.abs() > 2 * dev
        left_out = 1.0 - float(sure.double().mean())
        assert left_out < 0.05, left_out
        assert torch.equal((amp > 0)[sure], (want > 0)[sure])
        out[f"dev_amp16_{i}"], out[f"std_{i}"], out[f"left_out_{i}"] = dev, float(want.std()), left_out
        out[f"dev_quant_{i}"] = float((q - want).abs().max())
        assert torch.equal(q, q.float().double())
        quant[f"quant_{i}"] = q.float().numpy()
        (out if i == 0 else frame)[f"logits64_{i}"] = want.numpy()
        print(f"net {H} x {W}: std {out[f'std_{i}']:.3f}  dev_amp16 {dev:.3e}  dev_quant {out[f'dev_quant_{i}']:.3e}  "
              f"left out {left_out:.4f}")
    np.savez_compressed(os.path.join(HERE, "g17_unet.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "g17_unet_frame.npz"), **frame)
    np.savez_compressed(os.path.join(HERE, "g17_unet_quant.npz"), **quant)


if __name__ == "__main__":
    main()
