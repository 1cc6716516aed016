"""Float64 restatement of the ray-drop U-Net contract of csrc/unet.hip (include/lidarnerf_hip.h, lnh_unet_*) from
torch functional ops: the blocks of lidarnvs/unet.py (DoubleConv, Down, Up with the transposed convolution, OutConv) and the whole
UNet(10, 1, bilinear=False) in eval mode.  With quantize=True weights and activations are rounded to fp16 exactly where the kernels
round them (packed input, every 3 x 3 convolution's output, every transposed convolution's output) and the BatchNorm + ReLU
epilogue runs in fp32 — the product sums stay float64, which is the one place this differs from the kernels' fp32 accumulation.

Also here, written once for the maker of golden G17 and the tests: the closed-form integer hash every weight, BatchNorm statistic
and input of G17 comes from (31 M parameters cannot be committed), and the integer-valued problems of the exact tests."""
import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (64, 128, 256, 512, 1024)
EPS = 1e-5
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


# ---- state-dict names and shapes of the reference's UNet(n_channels, 1, bilinear=False), in its order ------------------------------
def _double_conv_spec(prefix, cin, cout):
    out = []
    for conv, bn, ci in (("0", "1", cin), ("3", "4", cout)):
        out.append((f"{prefix}.{conv}.weight", (cout, ci, 3, 3)))
        out += [(f"{prefix}.{bn}.{k}", () if k == "num_batches_tracked" else (cout,)) for k in BN_KEYS]
    return out


def state_spec(n_channels=10):
    spec = _double_conv_spec("inc.double_conv", n_channels, 64)
    for i in range(4):
        spec += _double_conv_spec(f"down{i + 1}.maxpool_conv.1.double_conv", CHANNELS[i], CHANNELS[i + 1])
    for i in range(4):
        cin = CHANNELS[4 - i]
        spec += [(f"up{i + 1}.up.weight", (cin, cin // 2, 2, 2)), (f"up{i + 1}.up.bias", (cin // 2,))]
        spec += _double_conv_spec(f"up{i + 1}.conv.double_conv", cin, cin // 2)
    spec += [("outc.conv.weight", (1, 64, 1, 1)), ("outc.conv.bias", (1,))]
    return spec


# ---- the hash: uniform numbers in [0, 1) from (tensor index, element index), NumPy uint64 arithmetic (wrapping) ----------------------
def hash_u01(tensor_index, count):
    """float64 [count]: element e of tensor t is mix(t * 0x9E3779B97F4A7C15 + e * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) >> 11,
    over 2^53, with mix the splitmix64 finaliser."""
    with np.errstate(over="ignore"):
        x = (np.uint64(tensor_index) * np.uint64(0x9E3779B97F4A7C15) + np.arange(count, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)
             + np.uint64(0x2545F4914F6CDD1D))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def hash_tensor(tensor_index, name, shape):
    """The G17 rule for one state-dict entry, float32 (what a checkpoint holds).  3 x 3 weights: uniform within the Kaiming bound
    sqrt(6 / (9 Cin)); transposed-convolution weights [Cin, Cout, 2, 2] within sqrt(3 / Cin) (no ReLU follows: unit gain); the
    head within sqrt(3 / 64); BatchNorm gamma in [0.8, 1.2], running_var in [0.5, 1.5]; beta, running_mean and biases in +-0.2."""
    n = int(np.prod(shape)) if len(shape) else 1
    u = hash_u01(tensor_index, n).reshape(shape)
    if name.endswith("num_batches_tracked"):
        return torch.zeros((), dtype=torch.int64)
    if name.endswith("running_var"):
        v = 0.5 + u
    elif name.endswith(("running_mean", "bias")):
        v = 0.4 * u - 0.2
    elif len(shape) == 1:  # BatchNorm weight
        v = 0.8 + 0.4 * u
    elif ".up." in name:
        v = (2 * u - 1) * np.sqrt(3.0 / shape[0])
    elif name.startswith("outc"):
        v = (2 * u - 1) * np.sqrt(3.0 / shape[1])
    else:
        v = (2 * u - 1) * np.sqrt(6.0 / (9 * shape[1]))
    return torch.from_numpy(np.asarray(v, np.float32))


def hash_state_dict(n_channels=10, first_index=0):
    return {name: hash_tensor(first_index + i, name, shape) for i, (name, shape) in enumerate(state_spec(n_channels))}


def hash_input(tensor_index, N, C, H, W):
    """float32 [N, C, H, W] in [-1, 1), channel 1 (depth) in [0, 80)."""
    x = 2 * hash_u01(tensor_index, N * C * H * W).reshape(N, C, H, W) - 1
    if C > 1:
        x[:, 1] = 40 * (x[:, 1] + 1)
    return torch.from_numpy(x.astype(np.float32))


INPUT_INDEX = 1000  # tensor indices of the G17 inputs: INPUT_INDEX + k


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def q16(x):
    """Round a float64 tensor to fp16 (nearest even) and back."""
    return x.to(torch.float16).to(torch.float64)


def q32(x):
    return x.to(torch.float32).to(torch.float64)


def bn_scale_shift(gamma, beta, mean, var, eps=None):
    """s = gamma / sqrt(var + eps), t = beta - mean s in float64 (lidarnerf/unet.py rounds both to fp32 once, at pack time)."""
    s = gamma.double() / torch.sqrt(var.double() + (EPS if eps is None else eps))
    return s, beta.double() - mean.double() * s


def conv_bn_relu(x, weight, gamma, beta, mean, var, quantize=False):
    """x float64 [N, Cin, H, W] (already fp16 values when quantize) -> relu(bn(conv3x3(x))) float64."""
    w = weight.double()
    s, t = bn_scale_shift(gamma, beta, mean, var)
    if quantize:
        w, s, t = q16(w), q32(s), q32(t)
    acc = F.conv2d(x, w, padding=1)
    if quantize:
        y = q32(q32(acc) * s[None, :, None, None] + t[None, :, None, None])  # (fmaf: one rounding; the product is exact in float64)
        y = q16(torch.relu(y))
    else:
        y = torch.relu(acc * s[None, :, None, None] + t[None, :, None, None])
    return y


def _bn(sd, prefix):
    return [sd[f"{prefix}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")]


def double_conv(sd, prefix, x, quantize=False):
    x = conv_bn_relu(x, sd[f"{prefix}.0.weight"], *_bn(sd, f"{prefix}.1"), quantize=quantize)
    return conv_bn_relu(x, sd[f"{prefix}.3.weight"], *_bn(sd, f"{prefix}.4"), quantize=quantize)


def down(sd, prefix, x, quantize=False):
    return double_conv(sd, f"{prefix}.maxpool_conv.1.double_conv", F.max_pool2d(x, 2), quantize)


def upconv(x, weight, bias, quantize=False):
    w, b = weight.double(), bias.double()
    if quantize:
        w = q16(w)
    y = F.conv_transpose2d(x, w, stride=2)
    if quantize:
        return q16(q32(q32(y) + b[None, :, None, None]))
    return y + b[None, :, None, None]


def up(sd, prefix, x1, x2, quantize=False):
    x1 = upconv(x1, sd[f"{prefix}.up.weight"], sd[f"{prefix}.up.bias"], quantize)
    dy, dx = x2.shape[2] - x1.shape[2], x2.shape[3] - x1.shape[3]
    x1 = F.pad(x1, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
    return double_conv(sd, f"{prefix}.conv.double_conv", torch.cat([x2, x1], dim=1), quantize)


def head(x, weight, bias, quantize=False):
    w = q16(weight.double()) if quantize else weight.double()
    y = F.conv2d(x, w) + bias.double()[None, :, None, None]
    return q32(y) if quantize else y


def prepare_input(images, quantize=False):
    x = images.double()
    return q16(x) if quantize else x


def unet_forward(sd, images, quantize=False):
    """Logits float64 [N, 1, H, W] of UNet(C, 1, bilinear=False).eval() with state dict `sd` on images [N, C, H, W]."""
    x1 = double_conv(sd, "inc.double_conv", prepare_input(images, quantize), quantize)
    x2 = down(sd, "down1", x1, quantize)
    x3 = down(sd, "down2", x2, quantize)
    x4 = down(sd, "down3", x3, quantize)
    x5 = down(sd, "down4", x4, quantize)
    x = up(sd, "up1", x5, x4, quantize)
    x = up(sd, "up2", x, x3, quantize)
    x = up(sd, "up3", x, x2, quantize)
    x = up(sd, "up4", x, x1, quantize)
    return head(x, sd["outc.conv.weight"], sd["outc.conv.bias"], quantize)


# ---- integer-valued problems: every product sum and every fp16 output exact ----------------------------------------------------------
def _choice(u, values):
    v = np.asarray(values, np.float64)
    return v[np.minimum((u * len(v)).astype(np.int64), len(v) - 1)]


def sparse_weight(tensor_index, shape, nnz_per_row, fan_in, two_share=0.25):
    """float32 weights in {-2 .. 2}: an element is non-zero with probability nnz_per_row / fan_in; +-2 for `two_share` of those."""
    n = int(np.prod(shape))
    u, v = hash_u01(tensor_index, n), hash_u01(tensor_index + 500000, n)
    w = np.where(u < nnz_per_row / fan_in, _choice(v, [-1, 1, -1, 1]) * np.where(hash_u01(tensor_index + 700000, n) < two_share, 2, 1), 0)
    return torch.from_numpy(w.reshape(shape).astype(np.float32))


def integer_image(tensor_index, shape, top=3):
    """float32 integers 0 .. top."""
    n = int(np.prod(shape))
    return torch.from_numpy(np.floor(hash_u01(tensor_index, n) * (top + 1)).reshape(shape).astype(np.float32))


def integer_bn(tensor_index, cout, scales, shift_step=0.25, shift_top=2.0):
    """(scale, shift) float32 [cout]: scales drawn from `scales` (powers of two), shifts multiples of shift_step in +-shift_top."""
    s = _choice(hash_u01(tensor_index, cout), scales)
    k = int(round(shift_top / shift_step))
    t = (np.floor(hash_u01(tensor_index + 300000, cout) * (2 * k + 1)) - k) * shift_step
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(t.astype(np.float32))


def integer_state_dict(n_channels=10, first_index=2000, nnz=2.0):
    """An integer-valued whole net: sparse weights in {-2 .. 2} with about `nnz` non-zeros per output channel, BatchNorm reduced to
    (scale, shift) with scale 0.5 in the first and 2 in the second convolution of every DoubleConv (so an output's granularity is
    its block input's), integer shifts and biases.  running_mean = 0, running_var = 1, and the tests set the BatchNorm eps to 0 (integer_unet_forward
    here, the modules' eps attribute there), so scale = gamma and shift = beta exactly."""
    sd = {}
    for i, (name, shape) in enumerate(state_spec(n_channels)):
        k = first_index + i
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros((), dtype=torch.int64)
        elif len(shape) == 4 and shape[2] == 3:
            sd[name] = sparse_weight(k, shape, nnz, 9 * shape[1])
        elif len(shape) == 4 and shape[2] == 2:
            sd[name] = sparse_weight(k, shape, nnz, shape[0])
        elif len(shape) == 4:
            sd[name] = sparse_weight(k, shape, 24, shape[1])
        elif name.endswith(".up.bias") or name.endswith("conv.bias"):
            sd[name] = torch.from_numpy(np.floor(hash_u01(k, shape[0]) * 3).astype(np.float32))
        elif name.endswith("running_mean"):
            sd[name] = torch.zeros(shape)
        elif name.endswith("running_var"):
            sd[name] = torch.ones(shape)
        elif name.endswith(".weight"):  # gamma: the scale itself
            sd[name] = torch.full(shape, 0.5 if name.endswith(".1.weight") else 2.0)
        else:  # beta: the shift
            sd[name] = torch.from_numpy((np.floor(hash_u01(k, shape[0]) * 3) - 1).astype(np.float32))
    return sd


def integer_unet_forward(sd, images, quantize=False):
    """unet_forward with eps = 0 in the BatchNorm of an integer_state_dict (scale = gamma exactly)."""
    global EPS
    keep, EPS = EPS, 0.0
    try:
        return unet_forward(sd, images, quantize)
    finally:
        EPS = keep


# ---- golden G17: shapes and inputs shared by tests/golden/make_g17_unet.py and the tests --------------------------------------------
G17_SIZES = ((23, 37), (66, 1030))
G17_BLOCK_HW = (17, 19)
# block name -> (state-dict prefix in the whole net whose hashed tensors the block uses, input shapes)
G17_BLOCKS = {
    "double_conv": ("inc", [(1, 10, 17, 19)]),
    "down": ("down1", [(1, 64, 17, 19)]),
    "up": ("up4", [(1, 128, 8, 9), (1, 64, 17, 19)]),  # (x1 to upsample, skip x2): the skip is one row and one column larger
    "out_conv": ("outc", [(1, 64, 17, 19)]),
}


def g17_block_inputs(name):
    """float32 inputs of a G17 block: the network input rule for double_conv, activations in [0, 2) for the others."""
    k = INPUT_INDEX + 10 * (1 + list(G17_BLOCKS).index(name))
    shapes = G17_BLOCKS[name][1]
    if name == "double_conv":
        return [hash_input(k, *shapes[0])]
    return [torch.from_numpy((2 * hash_u01(k + j, int(np.prod(s)))).reshape(s).astype(np.float32)) for j, s in enumerate(shapes)]


def g17_image(size_index):
    H, W = G17_SIZES[size_index]
    return hash_input(INPUT_INDEX + size_index, 1, 10, H, W)


def block_forward(name, sd, inputs, quantize=False):
    """The restatement of one G17 block on float32 inputs, with the whole net's state dict."""
    xs = [prepare_input(x, quantize) for x in inputs]
    if name == "double_conv":
        return double_conv(sd, "inc.double_conv", xs[0], quantize)
    if name == "down":
        return down(sd, "down1", xs[0], quantize)
    if name == "up":
        return up(sd, "up4", xs[0], xs[1], quantize)
    return head(xs[0], sd["outc.conv.weight"], sd["outc.conv.bias"], quantize)


# ---- the same network from stock torch modules (the reference's formulation, written fresh): state-dict round trips ------------------
def stock_unet(n_channels=10):
    import torch.nn as nn

    class DoubleConv(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.double_conv = nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(True),
                                             nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(True))

        def forward(self, x):
            return self.double_conv(x)

    class Down(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), DoubleConv(cin, cout))

        def forward(self, x):
            return self.maxpool_conv(x)

    class Up(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.up = nn.ConvTranspose2d(cin, cin // 2, 2, stride=2)
            self.conv = DoubleConv(cin, cout)

        def forward(self, x1, x2):
            x1 = self.up(x1)
            x1 = F.pad(x1, [0, x2.shape[3] - x1.shape[3], 0, x2.shape[2] - x1.shape[2]])
            return self.conv(torch.cat([x2, x1], dim=1))

    class Out(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(64, 1, 1)

        def forward(self, x):
            return self.conv(x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.inc = DoubleConv(n_channels, 64)
            for i in range(4):
                setattr(self, f"down{i + 1}", Down(CHANNELS[i], CHANNELS[i + 1]))
            for i in range(4):
                setattr(self, f"up{i + 1}", Up(CHANNELS[4 - i], CHANNELS[3 - i]))
            self.outc = Out()

        def forward(self, x):
            xs = [self.inc(x)]
            for i in range(4):
                xs.append(getattr(self, f"down{i + 1}")(xs[-1]))
            y = xs[4]
            for i in range(4):
                y = getattr(self, f"up{i + 1}")(y, xs[3 - i])
            return self.outc(y)

    return Net()


# ---- integer problems of the single kernels (tests/test_unet_gpu.py; their exactness is asserted in tests/test_unet_cpu.py) ------
def conv_scale_shift_relu(x, w, s, t, quantize=False):
    """relu(conv3x3(x, w) * s + t) in float64; quantize: fp16 weights, fp32 epilogue, fp16 output."""
    w, s, t = w.double(), s.double(), t.double()
    acc = F.conv2d(x, q16(w) if quantize else w, padding=1)
    if quantize:
        return q16(torch.relu(q32(q32(acc) * s[None, :, None, None] + t[None, :, None, None])))
    return torch.relu(acc * s[None, :, None, None] + t[None, :, None, None])


# (C0 real channels, C1, Cout, output H, W, pool, (H - H1, W - W1), N); with pool the source is (2H + 1) x (2W + 1) except where noted
CONV_CASES = [
    (10, 0, 64, 16, 16, 0, None, 1), (10, 0, 64, 17, 31, 0, None, 2), (10, 0, 64, 35, 67, 0, None, 1),
    (64, 0, 128, 16, 16, 0, None, 2), (64, 0, 128, 17, 31, 0, None, 1), (64, 0, 128, 17, 33, 1, None, 2),
    (64, 0, 128, 16, 17, 1, None, 1), (64, 0, 64, 1, 257, 0, None, 1), (64, 0, 64, 15, 17, 0, None, 1),
    (64, 64, 64, 17, 31, 0, (0, 0), 2), (64, 64, 64, 17, 31, 0, (1, 0), 1), (64, 64, 64, 17, 31, 0, (0, 1), 1),
    (64, 64, 64, 17, 31, 0, (1, 1), 1), (64, 64, 64, 35, 67, 0, (1, 1), 1), (64, 64, 64, 16, 16, 0, (1, 1), 2),
    (512, 512, 512, 16, 16, 0, (0, 0), 1), (512, 512, 512, 17, 31, 0, (1, 1), 1), (96, 32, 64, 17, 31, 0, (1, 0), 1),
]


def conv_case(index):
    """Inputs and the float64 answer of CONV_CASES[index].  src0 f32 [N, C0, H0, W0] integers 0 .. 3, src1 f32 [N, C1, H1, W1] or
    None, weight f32 [Cout, C0 + C1, 3, 3] sparse in {-2 .. 2} (about 16 non-zeros per output channel), scale from {1/4, 1/2, 1, 2},
    shift a multiple of 1/4 in +-2; `want` = relu(conv(cat(pool(src0), pad(src1))) * scale + shift), `bound` = the largest sum of
    |products| of any output (exact in fp32 below 2^24)."""
    C0, C1, Cout, H, W, pool, off, N = CONV_CASES[index]
    k = 3000 + 20 * index
    H0, W0 = (2 * H + 1, 2 * W + (index % 2)) if pool else (H, W)
    src0 = integer_image(k, (N, C0, H0, W0))
    src1 = integer_image(k + 1, (N, C1, H - off[0], W - off[1])) if C1 else None
    w = sparse_weight(k + 2, (Cout, C0 + C1, 3, 3), 16, 9 * (C0 + C1))
    s, t = integer_bn(k + 3, Cout, [0.25, 0.5, 1.0, 2.0])
    x = F.max_pool2d(src0.double(), 2) if pool else src0.double()
    if C1:
        x = torch.cat([x, F.pad(src1.double(), [0, off[1], 0, off[0]])], dim=1)
    want = conv_scale_shift_relu(x, w, s, t)
    bound = float(F.conv2d(x.abs(), w.double().abs(), padding=1).max())
    return {"src0": src0, "src1": src1, "weight": w, "scale": s, "shift": t, "pool": pool, "x": x, "want": want, "bound": bound}


UPCONV_CASES = [(128, 64, 1, 2, 1), (128, 64, 4, 64, 1), (128, 64, 9, 17, 2), (1024, 512, 1, 2, 2), (1024, 512, 4, 64, 1),
                (1024, 512, 9, 17, 1)]


def upconv_case(index):
    """x f32 [N, Cin, H, W] integers 0 .. 3, weight f32 [Cin, Cout, 2, 2] sparse in {-2 .. 2}, integer bias in +-2."""
    Cin, Cout, H, W, N = UPCONV_CASES[index]
    k = 4000 + 20 * index
    x = integer_image(k, (N, Cin, H, W))
    w = sparse_weight(k + 1, (Cin, Cout, 2, 2), 16, Cin)
    b = torch.from_numpy((np.floor(hash_u01(k + 2, Cout) * 5) - 2).astype(np.float32))
    want = upconv(x.double(), w, b)
    bound = float(F.conv_transpose2d(x.double().abs(), w.double().abs(), stride=2).max()) + 2
    return {"x": x, "weight": w, "bias": b, "want": want, "bound": bound}


def head_case():
    """x f32 [2, 64, 17, 19] integers 0 .. 3, weight [1, 64, 1, 1] in {-2 .. 2}, bias 3; pixel (0, 0, 0) is arranged to give a logit of
    exactly 0 and pixel (0, 0, 1) holds a NaN."""
    x = integer_image(5000, (2, 64, 17, 19))
    w = sparse_weight(5001, (1, 64, 1, 1), 24, 64)
    w[0, 7, 0, 0] = -1.0
    b = torch.tensor([3.0])
    x[0, :, 0, 0] = 0
    x[0, 7, 0, 0] = 3
    x[0, 5, 0, 1] = float("nan")
    want = head(x.double(), w, b)
    return {"x": x, "weight": w, "bias": b, "want": want}
