"""Integer problems with one answer for the weight gradient of the ray-drop U-Net's 3 x 3 convolutions (csrc/unet_train_wgrad.hip;
DESIGN §19), torch on the CPU, shared by tests/test_unet_train_step_cpu.py and tests/test_unet_train_step_gpu.py.

Operands: X integers 0 .. 3 (unet_ref.integer_image), dz sparse integers -2 .. 2 (unet_ref.sparse_weight: a quarter of the elements
non-zero).  The answer is the float64 weight gradient of F.conv2d(cat(pool(src0), pad(src1)), W, padding=1); every partial sum of
|products| stays far below 2^24, so fp32 sums in any order give it exactly."""
import functools

import torch
import torch.nn.functional as F

import unet_ref as R

# (real Cin of source 0, C1, Cout, output H, W, source size with pool or None, (H - H1, W - W1) or None, N) — the smallest shapes at
# which each mechanism of the kernel can still go wrong:
WGRAD_CASES = [
    (10, 0, 64, 16, 16, None, None, 1),        # a  M = 256: whole steps, one slice; channels 10 .. 31 of the padded operand not written
    (10, 0, 64, 17, 31, None, None, 2),        # b  M = 1054: ragged last step, five slices, the image seam inside a step
    (64, 0, 128, 17, 33, (35, 67), None, 2),   # c  pooled, odd source rows and columns that no window covers
    (64, 0, 128, 16, 17, (33, 34), None, 2),   # c' pooled, an odd row only
    (64, 0, 64, 1, 257, None, None, 1),        # d  every vertical tap is all padding: six of the nine planes are exactly zero
    (64, 64, 64, 17, 31, None, (0, 0), 1),     # e  the zero-pad rule of the second source, every combination
    (64, 64, 64, 17, 31, None, (1, 0), 1),
    (64, 64, 64, 17, 31, None, (0, 1), 1),
    (64, 64, 64, 17, 31, None, (1, 1), 1),
    (512, 512, 512, 4, 6, None, (0, 0), 1),    # f  M = 24 < one step
    (1024, 0, 1024, 2, 3, None, None, 2),      # g  the largest gradient; the single-partial path
    (64, 0, 64, 41, 59, None, None, 1),        # h  M = 2419: ten slices, more than 8 — the one-thread-per-element finishing kernel
]
WGRAD_IDS = ["a", "b", "c", "c2", "d", "e00", "e10", "e01", "e11", "f", "g", "h"]


@functools.lru_cache(maxsize=None)
def wgrad_case(k):
    """src0 f32 [N, C0, H0, W0], src1 f32 [N, C1, H1, W1] or None, dz f32 [N, Cout, H, W], `x` the operand the convolution sees
    (float64 [N, C0 + C1, H, W]), `want` float64 [Cout, C0 + C1, 3, 3], `bound` the largest sum of |products| of any entry."""
    C0, C1, Cout, H, W, src, off, N = WGRAD_CASES[k]
    s = 7600 + 10 * k
    H0, W0 = src or (H, W)
    src0 = R.integer_image(s, (N, C0, H0, W0))
    src1 = R.integer_image(s + 1, (N, C1, H - off[0], W - off[1])) if C1 else None
    dz = R.sparse_weight(s + 2, (N, Cout, H, W), 1, 4)
    x = F.max_pool2d(src0.double(), 2) if src else src0.double()
    if C1:
        x = torch.cat([x, F.pad(src1.double(), [0, off[1], 0, off[0]])], dim=1)
    assert tuple(x.shape[2:]) == (H, W)
    return {"src0": src0, "src1": src1, "dz": dz, "pool": src is not None, "x": x, "want": weight_gradient(x, dz.double()),
            "bound": float(weight_gradient(x.abs(), dz.double().abs()).max())}


def weight_gradient(x, dz):
    """dW[co, ci, dy, dx] = sum_{n, y, x} dz[n, co, y, x] xpad[n, ci, y + dy, x + dx] in float64: the gradient of
    F.conv2d(x, W, padding=1) with respect to W for the cotangent dz."""
    return torch.nn.grad.conv2d_weight(x, (dz.shape[1], x.shape[1], 3, 3), dz, padding=1)
