"""Float64 restatement of the ray-drop U-Net in training mode, NumPy / torch on the CPU: the whole net's forward keeping
its state and its backward from that state with no autograd inside — layer backward through batch-statistics BatchNorm, concatenation
split with the crop, max-pool backward to the first maximum plus the skip gradient, transposed-convolution and head backward.
tests/test_unet_train_cpu.py holds it to autograd of the stock modules; tests/test_unet_train_gpu.py holds the kernels of
csrc/unet_train.hip (pool backward, head backward, the transposed convolution's data and weight gradient) to its formulas.

Also here: the hashed problems of the loss (golden G18) and the integer-valued problems of the exact kernel tests."""
import numpy as np
import torch
import torch.nn.functional as F

import unet_ref as R


# ---- loss and validation score: hashed problems shared by tests/golden/make_g18_unet_train.py and the tests --------------------------------
# (N, H, W, share of kept pixels in the mask, special)
LOSS_CASES = [(2, 17, 19, 0.7, None), (1, 16, 16, 0.5, None), (3, 5, 7, 0.9, "second image empty"), (2, 32, 48, 0.0, "all empty")]


def loss_case(k):
    """(logits f64 [N, H, W] in +-4, masks f64 [N, H, W] of 0 / 1).  "second image empty": image 1 has an all-zero mask and logits
    below zero — the pair of empty sets that evaluate()'s per-image score counts as 1; "all empty": the same for the whole batch."""
    N, H, W, keep, special = LOSS_CASES[k]
    n = N * H * W
    logits = torch.from_numpy((8 * R.hash_u01(9500 + k, n) - 4).reshape(N, H, W))
    masks = torch.from_numpy((R.hash_u01(9600 + k, n) < keep).astype(np.float64).reshape(N, H, W))
    if special == "second image empty":
        masks[1] = 0
        logits[1] = -logits[1].abs() - 0.5
    elif special == "all empty":
        logits = -logits.abs() - 0.5
    return logits, masks


# ---- golden G18, training-mode record: the batch, the cotangent and the names recorded -----------------------------------------------------
G18_RUNNING = ["inc.double_conv.1.running_mean", "inc.double_conv.1.running_var", "down4.maxpool_conv.1.double_conv.4.running_mean",
               "down4.maxpool_conv.1.double_conv.4.running_var", "up4.conv.double_conv.1.running_mean", "up4.conv.double_conv.1.running_var"]
G18_GRAD_NORMS = ["inc.double_conv.0.weight", "down4.maxpool_conv.1.double_conv.4.weight", "down4.maxpool_conv.1.double_conv.4.bias",
                  "up1.up.weight", "up4.conv.double_conv.3.weight", "outc.conv.weight"]


def g18_train_batch():
    """float32 [2, 10, 23, 37]: odd sizes, so every decoder level pads its upsampled tensor."""
    return torch.cat([R.g17_image(0), R.hash_input(1234, 1, 10, 23, 37)])


def g18_train_cotangent():
    """float64 [2, 1, 23, 37] in +-1."""
    return torch.from_numpy(np.where(R.hash_u01(9800, 2 * 23 * 37) < 0.5, -1.0, 1.0).reshape(2, 1, 23, 37))


# ---- the whole net in training mode, float64: forward keeping its state, and backward from that state ------------------------------------
# Written from the layer formulas above and torch functional ops, with no autograd: tests/test_unet_train_cpu.py holds it to autograd
# of the stock modules (unet_ref.stock_unet) in float64.  (No quantised form of the whole net yet: that belongs with the kernels.)
def _layer_forward(x, w, gamma, beta, eps):
    z = F.conv2d(x, w, padding=1)
    M = z.numel() // z.shape[1]
    mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    s = gamma * invstd
    a = torch.relu(z * s[None, :, None, None] + (beta - mean * s)[None, :, None, None])
    return a, {"x": x, "z": z, "a": a, "mean": mean, "var": var, "invstd": invstd, "s": s, "M": M}


def _layer_backward(st, w, da, need_dx=True):
    """(dx or None, dW, dgamma, dbeta) of conv -> BatchNorm(batch statistics) -> ReLU from the saved state."""
    g = da * (st["a"] > 0)
    xh = (st["z"] - st["mean"][None, :, None, None]) * st["invstd"][None, :, None, None]
    dbeta, dgamma = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    dz = st["s"][None, :, None, None] * (g - (dbeta / st["M"])[None, :, None, None] - xh * (dgamma / st["M"])[None, :, None, None])
    dW = torch.nn.grad.conv2d_weight(st["x"], w.shape, dz, padding=1)
    dx = F.conv_transpose2d(dz, w, padding=1) if need_dx else None
    return dx, dW, dgamma, dbeta


def pool_backward(x, dpool, dskip=None):
    """Gradient of MaxPool2d(2) at x [N, C, H0, W0] for dpool [N, C, H0 // 2, W0 // 2]: all of it to the first maximum of each 2 x 2
    window in row-major order; rows and columns the floor division left out get none; dskip (x's other use) is added."""
    N, C, H0, W0 = x.shape
    H, W = H0 // 2, W0 // 2
    win = x[:, :, :2 * H, :2 * W].reshape(N, C, H, 2, W, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W, 4)
    first = torch.zeros(N, C, H, W, dtype=torch.int64)
    best = win[..., 0]
    for k in range(1, 4):  # strict >: a later equal value does not take over; a NaN does (torch's rule)
        take = (win[..., k] > best) | torch.isnan(win[..., k])
        first = torch.where(take, torch.full_like(first, k), first)
        best = torch.where(take, win[..., k], best)
    routed = F.one_hot(first, 4).to(x.dtype) * dpool[..., None]
    dx = torch.zeros_like(x)
    dx[:, :, :2 * H, :2 * W] = routed.reshape(N, C, H, W, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * H, 2 * W)
    return dx if dskip is None else dx + dskip


def upconv_backward(x, w, dy):
    """(dx, dW, dbias) of ConvTranspose2d(kernel 2, stride 2): dx[p, ci] = sum_{q, co} dy[2p + q, co] W[ci, co, q], dW[ci, co, q] =
    sum_p x[p, ci] dy[2p + q, co], dbias = sum dy."""
    N, Co, H2, W2 = dy.shape
    d6 = dy.reshape(N, Co, H2 // 2, 2, W2 // 2, 2)
    return torch.einsum("nohawb,ioab->nihw", d6, w), torch.einsum("nihw,nohawb->ioab", x, d6), dy.sum((0, 2, 3))


_DC = ["inc.double_conv"] + [f"down{i}.maxpool_conv.1.double_conv" for i in range(1, 5)] + [f"up{i}.conv.double_conv" for i in range(1, 5)]


def unet_train_forward(sd, images, eps=1e-5, momentum=0.1):
    """(logits f64 [N, 1, H, W], state): UNet(C, 1, bilinear=False) in training mode on float64 copies of `sd`; state keeps every
    layer's saved tensors and `running`: the running statistics after this call."""
    sd = {k: v.double() for k, v in sd.items()}
    state = {"layers": [], "running": {}, "ups": []}

    def dc(prefix, x):
        for conv, bn in (("0", "1"), ("3", "4")):
            x, st = _layer_forward(x, sd[f"{prefix}.{conv}.weight"], sd[f"{prefix}.{bn}.weight"], sd[f"{prefix}.{bn}.bias"], eps)
            state["layers"].append(st)
            M = st["M"]
            state["running"][f"{prefix}.{bn}.running_mean"] = (1 - momentum) * sd[f"{prefix}.{bn}.running_mean"] + momentum * st["mean"]
            state["running"][f"{prefix}.{bn}.running_var"] = (1 - momentum) * sd[f"{prefix}.{bn}.running_var"] + \
                momentum * (st["var"] * (M / (M - 1.0)))
        return x

    xs = [dc(_DC[0], images.double())]
    for l in range(1, 5):
        xs.append(dc(_DC[l], F.max_pool2d(xs[-1], 2)))
    y = xs[4]
    for i in range(1, 5):
        skip = xs[4 - i]
        up = F.conv_transpose2d(y, sd[f"up{i}.up.weight"], stride=2) + sd[f"up{i}.up.bias"][None, :, None, None]
        state["ups"].append({"x": y, "size": up.shape[2:]})
        up = F.pad(up, [0, skip.shape[3] - up.shape[3], 0, skip.shape[2] - up.shape[2]])
        y = dc(_DC[4 + i], torch.cat([skip, up], dim=1))
    state["skips"], state["head_in"] = xs, y
    return F.conv2d(y, sd["outc.conv.weight"]) + sd["outc.conv.bias"][None, :, None, None], state


def unet_backward_from_state(sd, state, dlogits):
    """{parameter name: gradient f64} for the cotangent dlogits [N, 1, H, W]: a function of (parameters, saved state, dlogits) only."""
    sd = {k: v.double() for k, v in sd.items()}
    grads = {}
    d = dlogits.double()
    grads["outc.conv.weight"] = (d * state["head_in"]).sum((0, 2, 3)).reshape(1, -1, 1, 1)
    grads["outc.conv.bias"] = d.sum().reshape(1)
    d = d * sd["outc.conv.weight"].reshape(1, -1, 1, 1)

    def dc_backward(index, d, first=False):
        prefix = _DC[index]
        for k, (conv, bn) in ((1, ("3", "4")), (0, ("0", "1"))):
            d, dW, dgamma, dbeta = _layer_backward(state["layers"][2 * index + k], sd[f"{prefix}.{conv}.weight"], d,
                                                   need_dx=not (first and k == 0))
            grads[f"{prefix}.{conv}.weight"], grads[f"{prefix}.{bn}.weight"], grads[f"{prefix}.{bn}.bias"] = dW, dgamma, dbeta
        return d

    dskips = [None] * 4
    for i in range(4, 0, -1):  # up4 .. up1
        dcat = dc_backward(4 + i, d)
        c0 = state["skips"][4 - i].shape[1]
        dskips[4 - i] = dcat[:, :c0]
        h2, w2 = state["ups"][i - 1]["size"]
        d, grads[f"up{i}.up.weight"], grads[f"up{i}.up.bias"] = upconv_backward(state["ups"][i - 1]["x"], sd[f"up{i}.up.weight"],
                                                                               dcat[:, c0:, :h2, :w2])
    for l in range(4, 0, -1):  # down4 .. down1: d is the gradient of x_l
        d = pool_backward(state["skips"][l - 1], dc_backward(l, d), dskips[l - 1])
    dc_backward(0, d, first=True)
    return grads


# ---- integer-valued problems of the kernel tests (exact in fp16 and in fp32 sums) ----------------------------------------------------------
# (N, C, H0, W0, channels per pixel of the skip-gradient tensor or 0 for none)
POOL_CASES = [(2, 32, 7, 9, 0), (1, 64, 16, 17, 64), (1, 64, 17, 16, 128), (2, 128, 5, 4, 160), (1, 32, 2, 2, 0), (1, 1024, 4, 6, 1024),
              (1, 64, 33, 67, 128)]


def pool_case(k):
    """x integers 0 .. 3 (most windows tie; image 0's first channel all zero), dpool and dskip multiples of 1/4 in +-2 — every sum
    exact in fp16.  Returns NCHW float64 tensors x, dpool, dskip (all Cs channels, or None) and want = pool_backward(x, dpool,
    dskip[:, :C])."""
    N, C, H0, W0, Cs = POOL_CASES[k]
    x = R.integer_image(9900 + 10 * k, (N, C, H0, W0)).double()
    x[0, 0] = 0
    dpool = (R.integer_image(9901 + 10 * k, (N, C, H0 // 2, W0 // 2), top=16).double() - 8) / 4
    dskip = (R.integer_image(9902 + 10 * k, (N, Cs, H0, W0), top=16).double() - 8) / 4 if Cs else None
    return {"x": x, "dpool": dpool, "dskip": dskip, "want": pool_backward(x, dpool, None if dskip is None else dskip[:, :C])}


HEAD_CASES = [(2, 17, 19), (1, 1, 64), (1, 5, 13), (3, 16, 16), (1, 66, 130)]


def head_backward_case(k):
    """a integers 0 .. 3 [N, 64, H, W], weight [64] in {-2 .. 2}, dlogits multiples of 1/4 in +-2 [N, 1, H, W]; want_dx = dlogit w,
    want_dweight = sum dlogit a, want_dbias = sum dlogit — the head's part of unet_backward_from_state, all exact in fp32."""
    N, H, W = HEAD_CASES[k]
    a = R.integer_image(9950 + 10 * k, (N, 64, H, W)).double()
    w = R.sparse_weight(9951 + 10 * k, (64,), 24, 64).double()
    d = (R.integer_image(9952 + 10 * k, (N, 1, H, W), top=16).double() - 8) / 4
    return {"a": a, "weight": w, "dlogits": d, "want_dx": d * w.reshape(1, 64, 1, 1), "want_dweight": (d * a).sum((0, 2, 3)),
            "want_dbias": d.sum().reshape(1), "bound": float((d.abs() * a).sum((0, 2, 3)).max())}


# (padding rows, columns of the gradient tensor beyond 2H x 2W; channels in front of the transposed convolution's; channels behind)
UPCONV_BWD_EMBED = [(0, 0, 0, 0), (1, 1, 64, 0), (1, 0, 128, 8), (0, 1, 512, 0), (0, 0, 64, 64), (1, 1, 512, 0)]


def upconv_backward_case(k):
    """The data gradient of unet_ref.UPCONV_CASES[k] (its x shape and weight): dy integers -2 .. 2 [N, Cout, 2H, 2W], embedded as
    channels [front, front + Cout) of `dcat` [N, front + Cout + behind, 2H + rows, 2W + cols] whose every other value is 3 (reading
    one of them would show); want_dx = upconv_backward(...)[0], `bound` its largest sum of |products| (exact in fp32 below 2^24)."""
    Cin, Cout, H, W, N = R.UPCONV_CASES[k]
    rows, cols, front, behind = UPCONV_BWD_EMBED[k]
    w = R.sparse_weight(4000 + 20 * k + 1, (Cin, Cout, 2, 2), 16, Cin).double()
    dy = R.integer_image(9980 + k, (N, Cout, 2 * H, 2 * W), top=4).double() - 2
    dcat = torch.full((N, front + Cout + behind, 2 * H + rows, 2 * W + cols), 3.0, dtype=torch.float64)
    dcat[:, front:front + Cout, :2 * H, :2 * W] = dy
    want = upconv_backward(torch.zeros(N, Cin, H, W, dtype=torch.float64), w, dy)[0]
    bound = float(upconv_backward(torch.zeros(N, Cin, H, W, dtype=torch.float64), w.abs(), dy.abs())[0].max())
    x = R.upconv_case(k)["x"].double()
    _, want_dw, want_db = upconv_backward(x, w, dy)
    bound_w = float(upconv_backward(x, w, dy.abs())[1].max())
    return {"weight": w, "x": x, "dy": dy, "dcat": dcat, "front": front, "want_dx": want, "bound": bound, "want_dweight": want_dw,
            "want_dbias": want_db, "bound_w": max(bound_w, float(dy.abs().sum((0, 2, 3)).max()))}


# ---- golden G18, blocks: the reference's DoubleConv / Down / Up / OutConv in train() mode, N = 2, 17 x 19 ---------------------------------
# block -> (prefix in the whole net whose hashed tensors it uses, prefix of its DoubleConv inside the block module or None, input shapes)
G18_BLOCKS = {
    "double_conv": ("inc", "double_conv", [(2, 10, 17, 19)]),
    "down": ("down1", "maxpool_conv.1.double_conv", [(2, 64, 17, 19)]),
    "up": ("up4", "conv.double_conv", [(2, 128, 8, 9), (2, 64, 17, 19)]),  # (x1 to upsample, skip x2 one row and column larger)
    "out_conv": ("outc", None, [(2, 64, 17, 19)]),
}


def g18_block_inputs(name):
    """float32 inputs: the network input rule for double_conv, activations in [0, 2) for the others."""
    k = 9850 + 10 * list(G18_BLOCKS).index(name)
    shapes = G18_BLOCKS[name][2]
    if name == "double_conv":
        return [R.hash_input(k, *shapes[0])]
    return [torch.from_numpy((2 * R.hash_u01(k + j, int(np.prod(s)))).reshape(s).astype(np.float32)) for j, s in enumerate(shapes)]


def g18_block_cotangent(name, shape):
    k = 9890 + list(G18_BLOCKS).index(name)
    return torch.from_numpy(np.where(R.hash_u01(k, int(np.prod(shape))) < 0.5, -1.0, 1.0).reshape(tuple(shape)))


def block_train(name, bsd, inputs, eps=1e-5, momentum=0.1):
    """One block in training mode from the layer formulas, float64, no autograd.  bsd: the block module's own state dict.  Returns
    (output, backward) with backward(cotangent) -> (parameter gradients by the module's names, input gradients); and the running
    statistics after the call under key "running" of the third value."""
    bsd = {k: v.double() for k, v in bsd.items()}
    xs = [x.double() for x in inputs]
    if name == "out_conv":
        w = bsd["conv.weight"]
        out = F.conv2d(xs[0], w) + bsd["conv.bias"][None, :, None, None]

        def backward(d):
            return {"conv.weight": (d * xs[0]).sum((0, 2, 3)).reshape(w.shape), "conv.bias": d.sum().reshape(1)}, \
                [d * w.reshape(1, -1, 1, 1)]
        return out, backward, {}
    dc = G18_BLOCKS[name][1]
    if name == "double_conv":
        x = xs[0]
    elif name == "down":
        x = F.max_pool2d(xs[0], 2)
    else:
        up = F.conv_transpose2d(xs[0], bsd["up.weight"], stride=2) + bsd["up.bias"][None, :, None, None]
        size = up.shape[2:]
        x = torch.cat([xs[1], F.pad(up, [0, xs[1].shape[3] - up.shape[3], 0, xs[1].shape[2] - up.shape[2]])], dim=1)
    states, running = [], {}
    for conv, bn in (("0", "1"), ("3", "4")):
        x, st = _layer_forward(x, bsd[f"{dc}.{conv}.weight"], bsd[f"{dc}.{bn}.weight"], bsd[f"{dc}.{bn}.bias"], eps)
        states.append(st)
        M = st["M"]
        running[f"{dc}.{bn}.running_mean"] = (1 - momentum) * bsd[f"{dc}.{bn}.running_mean"] + momentum * st["mean"]
        running[f"{dc}.{bn}.running_var"] = (1 - momentum) * bsd[f"{dc}.{bn}.running_var"] + momentum * (st["var"] * (M / (M - 1.0)))

    def backward(d):
        grads = {}
        for k, (conv, bn) in ((1, ("3", "4")), (0, ("0", "1"))):
            d, dW, dgamma, dbeta = _layer_backward(states[k], bsd[f"{dc}.{conv}.weight"], d)
            grads[f"{dc}.{conv}.weight"], grads[f"{dc}.{bn}.weight"], grads[f"{dc}.{bn}.bias"] = dW, dgamma, dbeta
        if name == "double_conv":
            return grads, [d]
        if name == "down":
            return grads, [pool_backward(xs[0], d)]
        c0 = xs[1].shape[1]
        dx1, grads["up.weight"], grads["up.bias"] = upconv_backward(xs[0], bsd["up.weight"], d[:, c0:, :size[0], :size[1]])
        return grads, [dx1, d[:, :c0]]
    return x, backward, running


# ---- golden G18, the training record: one fixed batch, 16 steps of the reference's loop --------------------------------------------------
G18_STEPS = 16


def g18_record_batch():
    """(images f32 [2, 10, 32, 48], masks f32 [2, 32, 48]): the mask is a function of the input, (depth < 50) & (channel 0 > -0.5)."""
    x = R.hash_input(9840, 2, 10, 32, 48)
    return x, ((x[:, 1] < 50) & (x[:, 0] > -0.5)).float()
