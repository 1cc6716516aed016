"""Problems and a quantised restatement of the training-mode convolution layer of the ray-drop U-Net (csrc/unet_train_conv.hip, the RAW
epilogue of csrc/unet.hip), NumPy / torch on the CPU, shared by tests/test_unet_train_conv_cpu.py and
tests/test_unet_train_conv_gpu.py.

The restatement rounds to fp16 where the kernels round (weights, z, a, every activation gradient) and to f32 where they keep f32
(mean, invstd, scale, shift, xhat, the products g xhat, dgamma, dbeta and the chain of dz); every sum is float64.  With quantize=False
it is tests/unet_train_ref.py's float64 layer."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import unet_ref as R
import unet_train_ref as T

q16, q32 = R.q16, R.q32


def _b(v):
    return v[None, :, None, None]


# ---- one layer, NCHW float64 tensors --------------------------------------------------------------------------------------------------
def layer_forward(x, w, gamma, beta, eps, quantize=True):
    """conv -> BatchNorm on the batch's statistics -> ReLU.  quantize: z = fp16(fp32(acc)), the statistics are those of that z, every
    derived vector is formed in float64 and rounded once to f32, a = fp16(max(fmaf(z, scale, shift), 0))."""
    if not quantize:
        return T._layer_forward(x, w, gamma, beta, eps)
    z = q16(q32(F.conv2d(x, q16(w.double()), padding=1)))
    st = bn_forward(z, gamma.double(), beta.double(), eps)
    st["x"] = x
    return st["a"], st


def bn_forward(z, gamma, beta, eps):
    """The quantised BatchNorm + ReLU of fp16-valued z [N, C, H, W] in float64: what lnh_unet_bn_stats and lnh_unet_bn_relu compute."""
    M = z.numel() // z.shape[1]
    mean = z.sum((0, 2, 3)) / M
    var = ((z * z).sum((0, 2, 3)) / M - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    s = gamma * invstd
    shift = beta - mean * s
    a = q16(torch.relu(q32(z * _b(q32(s)) + _b(q32(shift)))))
    return {"z": z, "a": a, "mean": q32(mean), "var": var, "invstd": q32(invstd), "s": q32(s), "shift": q32(shift), "M": M,
            "mean64": mean, "invstd64": invstd}


def bn_backward(st, da):
    """(dz, dgamma, dbeta) of the quantised BatchNorm + ReLU: lnh_unet_bn_relu_backward's arithmetic, float64 sums."""
    M = st["M"]
    g = da * (st["a"] > 0)
    xh = q32(q32(st["z"] - _b(st["mean"])) * _b(st["invstd"]))
    dbeta, dgamma = q32(g.sum((0, 2, 3))), q32(q32(g * xh).sum((0, 2, 3)))
    inner = q32(q32(g - _b(q32(dbeta / M))) - q32(xh * _b(q32(dgamma / M))))
    return q16(q32(_b(st["s"]) * inner)), dgamma, dbeta


def layer_backward(st, w, da, need_dx=True, quantize=True):
    """(dx or None, dgamma, dbeta, dz) from the saved state; quantize: dx = fp16(fp32(conv_transpose(dz, fp16(w))))."""
    if not quantize:
        dx, _, dgamma, dbeta = T._layer_backward(st, w, da, need_dx)
        return dx, dgamma, dbeta, None
    dz, dgamma, dbeta = bn_backward(st, da)
    dx = q16(q32(F.conv_transpose2d(dz, q16(w.double()), padding=1))) if need_dx else None
    return dx, dgamma, dbeta, dz


# ---- the whole net ---------------------------------------------------------------------------------------------------------------------
def unet_train_forward(sd, images, eps=1e-5, quantize=True):
    """(logits, state) of the net in training mode with the layer above; quantize=False: unet_train_ref.unet_train_forward's values."""
    sd = {k: v.double() for k, v in sd.items()}
    qa = q16 if quantize else (lambda t: t)
    state = {"layers": [], "ups": []}

    def dc(prefix, x):
        for conv, bn in (("0", "1"), ("3", "4")):
            x, st = layer_forward(x, sd[f"{prefix}.{conv}.weight"], sd[f"{prefix}.{bn}.weight"], sd[f"{prefix}.{bn}.bias"], eps, quantize)
            state["layers"].append(st)
        return x

    xs = [dc(T._DC[0], qa(images.double()))]
    for l in range(1, 5):
        xs.append(dc(T._DC[l], F.max_pool2d(xs[-1], 2)))
    y = xs[4]
    for i in range(1, 5):
        skip = xs[4 - i]
        up = R.upconv(y, sd[f"up{i}.up.weight"], sd[f"up{i}.up.bias"], quantize)
        state["ups"].append({"x": y, "size": up.shape[2:]})
        up = F.pad(up, [0, skip.shape[3] - up.shape[3], 0, skip.shape[2] - up.shape[2]])
        y = dc(T._DC[4 + i], torch.cat([skip, up], dim=1))
    state["skips"], state["head_in"] = xs, y
    return R.head(y, sd["outc.conv.weight"], sd["outc.conv.bias"], quantize), state


def unet_train_backward(sd, state, dlogits, quantize=True):
    """{name: gradient} of the 46 tensors lidarnerf.unet_train.train_backward returns, in unet_backward_from_state's order."""
    sd = {k: v.double() for k, v in sd.items()}
    qa = q16 if quantize else (lambda t: t)
    qw = (lambda t: q16(t)) if quantize else (lambda t: t)
    grads = {}
    d = dlogits.double()
    grads["outc.conv.weight"] = (d * state["head_in"]).sum((0, 2, 3)).reshape(1, -1, 1, 1)
    grads["outc.conv.bias"] = d.sum().reshape(1)
    d = qa(d * qw(sd["outc.conv.weight"]).reshape(1, -1, 1, 1))

    def dc_backward(index, d, first=False):
        prefix = T._DC[index]
        for k, (conv, bn) in ((1, ("3", "4")), (0, ("0", "1"))):
            d, dgamma, dbeta, _ = layer_backward(state["layers"][2 * index + k], sd[f"{prefix}.{conv}.weight"], d,
                                                 need_dx=not (first and k == 0), quantize=quantize)
            grads[f"{prefix}.{bn}.weight"], grads[f"{prefix}.{bn}.bias"] = dgamma, dbeta
        return d

    dskips = [None] * 4
    for i in range(4, 0, -1):
        dcat = dc_backward(4 + i, d)
        c0 = state["skips"][4 - i].shape[1]
        dskips[4 - i] = dcat[:, :c0]
        h2, w2 = state["ups"][i - 1]["size"]
        d, grads[f"up{i}.up.weight"], grads[f"up{i}.up.bias"] = T.upconv_backward(state["ups"][i - 1]["x"], qw(sd[f"up{i}.up.weight"]),
                                                                               dcat[:, c0:, :h2, :w2])
        d = qa(d)
    for l in range(4, 0, -1):
        d = qa(T.pool_backward(state["skips"][l - 1], dc_backward(l, d), dskips[l - 1]))
    dc_backward(0, d, first=True)
    return grads


GRAD_NAMES = [n for n, s in R.state_spec() if n.endswith((".weight", ".bias")) and not (len(s) == 4 and s[2] == 3)]


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
PACK_CASES = [(64, 10), (64, 64), (128, 64), (64, 128), (1024, 1024)]  # (Cout, Cin)


def pack_weight(k):
    Cout, Cin = PACK_CASES[k]
    n = Cout * Cin * 9
    return torch.from_numpy((R.hash_u01(7000 + k, n) * 2 - 1).astype(np.float32).reshape(Cout, Cin, 3, 3))


def pack_images(w):
    """(fwd fp16 [Cout, 9, Cpad], bwd fp16 [Cin, 9, Cout]) by torch indexing."""
    Cout, Cin = w.shape[:2]
    cpad = 32 if Cin <= 32 else Cin
    fwd = torch.zeros(Cout, 9, cpad, dtype=torch.float16)
    fwd[:, :, :Cin] = w.reshape(Cout, Cin, 9).permute(0, 2, 1).to(torch.float16)
    bwd = w.reshape(Cout, Cin, 9).flip(2).permute(1, 2, 0).to(torch.float16).contiguous()
    return fwd, bwd


# ---- the raw convolution as a data gradient: integer problems ------------------------------------------------------------------------
# (layer Cout = channels of dz, C0, C1 of the layer's operand, H, W, N)
DGRAD_CASES = [(64, 64, 0, 15, 17, 1), (128, 64, 64, 16, 16, 1), (1024, 512, 0, 2, 3, 1), (64, 64, 0, 1, 257, 1), (64, 64, 0, 9, 11, 2),
               (128, 64, 64, 17, 17, 1)]  # (the last: odd sizes, chained into pool_backward and upconv2x2_backward_data)


@functools.lru_cache(maxsize=None)
def dgrad_case(k):
    """dz integers -2 .. 2 [N, Cout, H, W], weight [Cout, C0 + C1, 3, 3] sparse in {-2 .. 2}; want = conv_transpose2d(dz, W, padding=1)
    [N, C0 + C1, H, W], `bound` its largest sum of |products| (exact in fp32 below 2^24)."""
    Cout, C0, C1, H, W, N = DGRAD_CASES[k]
    w = R.sparse_weight(7100 + 10 * k, (Cout, C0 + C1, 3, 3), 16, 9 * Cout).double()
    dz = R.integer_image(7101 + 10 * k, (N, Cout, H, W), top=4).double() - 2
    return {"weight": w, "dz": dz, "want": F.conv_transpose2d(dz, w, padding=1),
            "bound": float(F.conv_transpose2d(dz.abs(), w.abs(), padding=1).max())}


# ---- exact BatchNorm problems ---------------------------------------------------------------------------------------------------------
BN_CASES = [(2, 32), (64, 32), (66, 64), (4 * 15 * 17, 64), (4 * 15 * 17, 1024), (64, 96), ((1 << 14) + 2, 32)]  # (M, C)
BN_MOMENTUM = 0.5


@functools.lru_cache(maxsize=None)
def bn_case(k):
    """z[p, c] = m_c + sigma_c e[p, c] with e = +-1, exactly M / 2 of each sign per channel, m_c an integer in -3 .. 3, sigma_c a power of two
    in 1/4 .. 4, eps = 0, gamma a power of two in 1/2 .. 2, beta a multiple of 1/4 in +-2: mean = m, var = sigma^2, invstd = 1 / sigma, scale =
    gamma / sigma, shift = beta - m scale, a = relu(gamma e + beta), xhat = e — one value each.  da holds small integers arranged so that,
    per channel, the sum of g = da [a > 0] over the pixels with e = +1 is M u and over those with e = -1 is M w (u, w small integers, 0
    where a is nowhere positive): dbeta = M (u + w), dgamma = M (u - w), dz = scale (g - (u + w) - e (u - w)).  Everything float64
    [M, C] / [C]."""
    M, C = BN_CASES[k]
    s = 7200 + 10 * k
    order = np.argsort(R.hash_u01(s, M * C).reshape(M, C), axis=0)
    e = np.where(np.argsort(order, axis=0) < M // 2, 1.0, -1.0)  # rank below M / 2: exactly half of every column
    m = np.floor(R.hash_u01(s + 1, C) * 7) - 3
    sigma = R._choice(R.hash_u01(s + 2, C), [0.25, 0.5, 1, 2, 4])
    gamma = R._choice(R.hash_u01(s + 3, C), [0.5, 1, 2])
    beta = (np.floor(R.hash_u01(s + 4, C) * 17) - 8) / 4
    rm = (np.floor(R.hash_u01(s + 5, C) * 9) - 4) / 4
    rv = (np.floor(R.hash_u01(s + 6, C) * 8) + 1) / 4
    z = m + sigma * e
    scale = gamma / sigma
    shift = beta - m * scale
    a = np.maximum(gamma * e + beta, 0)
    da = np.floor(R.hash_u01(s + 7, M * C).reshape(M, C) * 7) - 3
    u = np.floor(R.hash_u01(s + 8, C) * 4) - 1
    w = np.floor(R.hash_u01(s + 9, C) * 4) - 2
    sums = []
    for sign, target in ((1.0, u), (-1.0, w)):
        sel = (e == sign) & (a > 0)
        n = sel.sum(0)
        want = np.where(n > 0, M * target, 0.0)
        delta = want - (da * sel).sum(0)
        q = np.where(n > 0, np.floor(delta / np.maximum(n, 1)), 0.0)
        r = delta - q * n  # 0 <= r < n
        rank = np.cumsum(sel, axis=0) - 1
        da = da + sel * (q + (rank < r))
        sums.append(want)
    g = da * (a > 0)
    dbeta, dgamma = sums[0] + sums[1], sums[0] - sums[1]
    dz = scale * (g - dbeta / M - e * (dgamma / M))
    t = torch.from_numpy
    return {"M": M, "C": C, "z": t(z), "e": t(e), "mean": t(m), "var": t(sigma * sigma), "invstd": t(1 / sigma), "gamma": t(gamma),
            "beta": t(beta), "scale": t(scale), "shift": t(shift), "a": t(a), "da": t(da), "dbeta": t(dbeta), "dgamma": t(dgamma),
            "dz": t(dz), "running_mean": t(rm), "running_var": t(rv), "want_running_mean": t(0.5 * rm + 0.5 * m),
            "want_running_var": t(0.5 * rv + 0.5 * (sigma * sigma * (M / (M - 1.0))))}


# ---- general data: hashed z, the float64 answer and the bounds of DESIGN §19 --------------------------------------------------------
GENERAL_BN = (2 * 23 * 37, 64)  # (M, C)


@functools.lru_cache(maxsize=None)
def bn_general_case():
    """z fp16-valued [M, C] = mean_c + sigma_c n (n roughly normal); channel 3 has |mean| = 100 sigma; da fp16-valued in +-2; gamma in
    [0.8, 1.2], beta in +-0.2 (f32-valued); eps = 1e-5."""
    M, C = GENERAL_BN
    n = (R.hash_u01(7400, M * C) + R.hash_u01(7401, M * C) + R.hash_u01(7402, M * C) - 1.5).reshape(M, C) * 2
    mean = 2 * R.hash_u01(7403, C) - 1
    sigma = 0.25 + R.hash_u01(7404, C)
    mean[3], sigma[3] = 50.0, 0.5
    z = q16(torch.from_numpy(mean + sigma * n))
    da = q16(torch.from_numpy(4 * R.hash_u01(7405, M * C).reshape(M, C) - 2))
    gamma = q32(torch.from_numpy(0.8 + 0.4 * R.hash_u01(7406, C)))
    beta = q32(torch.from_numpy(0.4 * R.hash_u01(7407, C) - 0.2))
    return {"z": z, "da": da, "gamma": gamma, "beta": beta, "eps": 1e-5}


E32, E53 = 2.0 ** -24, 2.0 ** -53


def bn_general_reference(c):
    """Float64 values of every output on the fp16-valued z / da of `c` and, under "bound", what the rounding model of DESIGN §19 allows
    a device output to differ from them.  The model: a float64 sum of M terms is off by at most M 2^-53 times the sum of |terms|; a
    value formed in float64 and rounded once to f32 by 2^-24 of itself; every fp32 operation of the backward by 2^-24 of its result."""
    z, da, gamma, beta, eps = c["z"], c["da"], c["gamma"], c["beta"], c["eps"]
    M = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)  # (the two-pass form: the reference does not cancel)
    invstd = 1 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    a = torch.relu(z * scale + shift)
    # sums: S1 = sum z, S2 = sum z^2 (terms exact), var = S2 / M - mean^2 cancels against mean z^2
    az, az2 = z.abs().mean(0), (z * z).mean(0)
    d_mean = (M + 2) * E53 * az
    d_var = (M + 4) * E53 * (az2 + mean * mean) + 2 * mean.abs() * d_mean
    r_inv = 0.5 * d_var / (var + eps) + 4 * E53  # relative, first order
    bound = {"mean": E32 * mean.abs() + d_mean, "invstd": invstd * (E32 + r_inv), "scale": scale.abs() * (E32 + r_inv + E53),
             "shift": E32 * shift.abs() + (mean * scale).abs() * (r_inv + 3 * E53) + scale.abs() * d_mean}
    # the backward: fp32 xhat from the f32 mean and invstd
    g = da * (a > 0)
    xh = (z - mean) * invstd
    d_xh = (E32 * mean.abs() + E32 * (z - mean).abs() + d_mean) * invstd + xh.abs() * (2 * E32 + r_inv)
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    bound["dbeta"] = E32 * dbeta.abs() + (M + 2) * E53 * g.abs().sum(0)
    bound["dgamma"] = E32 * dgamma.abs() + (g.abs() * d_xh).sum(0) + (E32 + (M + 2) * E53) * (g * xh).abs().sum(0)
    dz = scale * (g - dbeta / M - xh * dgamma / M)
    terms = g.abs() + dbeta.abs() / M + xh.abs() * dgamma.abs() / M
    d_inner = 6 * E32 * terms + d_xh * dgamma.abs() / M + (bound["dgamma"] * xh.abs() + bound["dbeta"]) / M
    bound["dz"] = 2.0 ** -11 * dz.abs() + 2.0 ** -25 + scale.abs() * d_inner * (1 + 2.0 ** -10) + dz.abs() * (2 * E32 + r_inv)
    return {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "a": a, "dbeta": dbeta, "dgamma": dgamma, "dz": dz,
            "bound": bound}
