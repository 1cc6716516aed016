"""The ray-drop U-Net of the mesh baselines on the device: inference of lidarnvs/unet.py's UNet(10, 1, bilinear=False) — the network
LidarNVSMeshing loads from a checkpoint and runs in predict_frame_with_raydrop (lidarnvs_meshing.py:28-41, 253-256) — through
the fused kernels of csrc/unet.hip (include/lidarnerf_hip.h, lnh_unet_*): fp16 NHWC activations, fp16 weights, fp32
accumulation, eval-mode BatchNorm + ReLU in fp32 in the convolution's epilogue, the 2 x 2 max-pool and the skip concatenation taken
on the operand read.  24 launches per forward, no framework op between them, no host read, no allocation after the first call of a
shape.  This is the reference's --amp arithmetic (torch.autocast) with one rounding per layer where autocast makes two.

Inference only: training the U-Net (raydrop_train_poisson.py) is not part of this package, and neither is bilinear=True.  No CPU
fallback."""
import torch
import torch.nn as nn

from . import _hip

CHANNELS = (64, 128, 256, 512, 1024)
_SYMBOLS = ("lnh_unet_workspace_size", "lnh_unet_input", "lnh_unet_conv3x3", "lnh_unet_upconv2x2", "lnh_unet_head")
MIN_SIZE = 16  # four halvings must leave a pixel


# ---- the entry points on tensors ----------------------------------------------------------------------------------------------------
def _nhwc(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float16 and t.dim() == 4 and t.is_contiguous()):
        raise RuntimeError(f"lidarnerf.unet: {what} must be a contiguous fp16 [N, H, W, C] GPU tensor")
    return t


def unet_input(images, out):
    """images f32 [N, C, H, W] (C <= 32) -> out fp16 [N, H, W, 32]."""
    _hip.require_cuda(images, out)
    N, C, H, W = images.shape
    if images.dtype != torch.float32 or tuple(_nhwc(out, "out").shape) != (N, H, W, 32):
        raise RuntimeError("lidarnerf.unet.unet_input: images f32 [N, C, H, W], out fp16 [N, H, W, 32]")
    _hip.call("lnh_unet_input", _hip.ptr(images), N, C, H, W, _hip.ptr(out))
    return out


def conv_operand(src0, src1, pool, out, what):
    """The source arguments of the three 3 x 3 entry points, (src0, C0, H0, W0, pool, src1, C1, H1, W1) as they take them, from src0
    [N, H0, W0, C0] (pool: its 2 x 2 maximum is read) and the optional src1 [N, H1, W1, C1]; then N, the channel count of `out` — the
    tensor `what` of the output's size [N, H, W, .] — and whether out and src1 fit src0's batch and output size."""
    N, H0, W0, C0 = _nhwc(src0, "src0").shape
    Cout = _nhwc(out, what).shape[3]
    H1 = W1 = C1 = 0
    if src1 is not None:
        _, H1, W1, C1 = _nhwc(src1, "src1").shape
    fits = tuple(out.shape[:3]) == ((N, H0 // 2, W0 // 2) if pool else (N, H0, W0)) and (src1 is None or src1.shape[0] == N)
    return (_hip.ptr(src0), C0, H0, W0, int(bool(pool)), _hip.ptr(src1), C1, H1, W1), N, Cout, fits


def conv3x3(src0, weight, scale, shift, out, src1=None, pool=False, tile=0):
    """lnh_unet_conv3x3: out [N, H, W, Cout] from src0 [N, H0, W0, C0] (pool: its 2 x 2 maximum) and the optional src1
    [N, H1, W1, C1]; weight fp16 [Cout, 9, C0 + C1], scale / shift f32 [Cout]."""
    operand, N, Cout, fits = conv_operand(src0, src1, pool, out, "out")
    if not fits or tuple(weight.shape) != (Cout, 9, operand[1] + operand[6]) or weight.dtype != torch.float16 or \
            scale.dtype != torch.float32 or shift.dtype != torch.float32 or scale.numel() != Cout or shift.numel() != Cout:
        raise RuntimeError("lidarnerf.unet.conv3x3: shapes of out / weight / scale / shift do not fit the sources")
    _hip.require_cuda(weight, scale, shift)
    _hip.call("lnh_unet_conv3x3", *operand, _hip.ptr(weight), _hip.ptr(scale), _hip.ptr(shift), N, Cout, int(tile), _hip.ptr(out))
    return out


def upconv2x2(x, weight, bias, out):
    """lnh_unet_upconv2x2: x [N, H, W, Cin] -> out [N, 2H, 2W, Cout]; weight fp16 [4, Cout, Cin], bias f32 [Cout]."""
    N, H, W, Cin = _nhwc(x, "x").shape
    Cout = _nhwc(out, "out").shape[3]
    if tuple(out.shape) != (N, 2 * H, 2 * W, Cout) or tuple(weight.shape) != (4, Cout, Cin) or weight.dtype != torch.float16 or \
            bias.dtype != torch.float32 or bias.numel() != Cout:
        raise RuntimeError("lidarnerf.unet.upconv2x2: shapes of out / weight / bias do not fit the input")
    _hip.require_cuda(weight, bias)
    _hip.call("lnh_unet_upconv2x2", _hip.ptr(x), N, H, W, Cin, _hip.ptr(weight), _hip.ptr(bias), Cout, _hip.ptr(out))
    return out


def head(x, weight, bias, logits, mask=None):
    """lnh_unet_head: x [N, H, W, 64] -> logits f32 [N, 1, H, W] and (optionally) mask f32 [N, 1, H, W] = logit > 0."""
    N, H, W, C = _nhwc(x, "x").shape
    if C != 64 or weight.numel() != 64 or weight.dtype != torch.float16 or bias.dtype != torch.float32 or bias.numel() != 1:
        raise RuntimeError("lidarnerf.unet.head: x [N, H, W, 64], weight fp16 [64], bias f32 [1]")
    for t in (logits, mask):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (N, 1, H, W)):
            raise RuntimeError(f"lidarnerf.unet.head: logits and mask must be f32 [{N}, 1, {H}, {W}]")
    _hip.require_cuda(weight, bias, logits, mask)
    _hip.call("lnh_unet_head", _hip.ptr(x), N, H, W, _hip.ptr(weight), _hip.ptr(bias), _hip.ptr(logits), _hip.ptr(mask))
    return logits


def level_sizes(H, W):
    return [(H >> l, W >> l) for l in range(5)]


def workspace_layout(N, H, W):
    """([(name, byte offset, shape [N, h, w, c])], total bytes) of the activation buffers of one forward: `input`, then mid{l} / x{l}
    of the encoder levels l = 0 .. 4, then up{l} / d{l} of the decoder levels l = 3 .. 0 (the decoder's DoubleConv reuses mid{l});
    every buffer 256-byte aligned.  The total equals lnh_unet_workspace_size(N, H, W)."""
    sizes = level_sizes(H, W)
    bufs = [("input", (N, H, W, 32))]
    for l, (h, w) in enumerate(sizes):
        bufs += [(f"mid{l}", (N, h, w, CHANNELS[l])), (f"x{l}", (N, h, w, CHANNELS[l]))]
    for l in range(4):
        h, w = sizes[l + 1]
        bufs += [(f"up{l}", (N, 2 * h, 2 * w, CHANNELS[l])), (f"d{l}", (N,) + sizes[l] + (CHANNELS[l],))]
    placed, total = place([(name, shape, torch.float16) for name, shape in bufs])
    return [e[:3] for e in placed], total


def _nbytes(shape, dtype):
    n = torch.empty(0, dtype=dtype).element_size()
    for d in shape:
        n *= d
    return n


def place(bufs):
    """[(name, shape, dtype)] -> ([(name, byte offset, shape, dtype)], total bytes): one after the other, each 256-byte aligned."""
    out, off = [], 0
    for name, shape, dtype in bufs:
        out.append((name, off, shape, dtype))
        off += (_nbytes(shape, dtype) + 255) // 256 * 256
    return out, off


def carve(raw, layout):
    """{name: view} of the buffers of a layout — entries (name, byte offset, shape[, dtype]), fp16 without a dtype — in the byte
    tensor `raw`."""
    views = {}
    for name, off, shape, *dtype in layout:
        dtype = dtype[0] if dtype else torch.float16
        views[name] = raw[off:off + _nbytes(shape, dtype)].view(dtype).view(shape)
    return views


def layer_table(n_channels=10, decoder_mid="mid"):
    """The 18 convolution layers in execution order, one dict each — the one statement of the net's topology; packing, inference and
    the training forward walk it forwards, the training backward in reverse.
      conv, bn       state-dict prefixes of the layer's Conv2d and BatchNorm2d
      src0, src1     buffer names of the operand; src1 None but for the concatenating layers
      pool           src0 is max-pooled 2 x 2 on read
      out            the activation buffer.  The first activation of decoder level l is `decoder_mid`{l}: inference reuses mid{l},
                     training keeps dmid{l} beside it (the backward needs both)
      level, cin (C0 + C1 of the parameter), cout
      up             None, or for a concatenating layer the block index i of the transposed convolution up{i + 1}.up (state-dict
                     prefix `up_name`) that makes src1 from the previous layer's activation
      dx             the buffer that receives the layer's data gradient: the previous layer's gradient buffer g{k - 1}, dcat{l} for a
                     concatenating layer, dpool{l} for a pooling one; None for layer 0
      dskip          for a pooling layer: the concatenation gradient whose first channels are the skip gradient of src0."""
    def pair(prefix, src0, src1, pool, mid, out, level, cin, dx, **more):
        c, k = CHANNELS[level], len(layers)
        return [dict(conv=f"{prefix}.0", bn=f"{prefix}.1", src0=src0, src1=src1, pool=pool, out=mid, level=level, cin=cin, cout=c,
                     up=None, dx=dx, **more),
                dict(conv=f"{prefix}.3", bn=f"{prefix}.4", src0=mid, src1=None, pool=False, out=out, level=level, cin=c, cout=c,
                     up=None, dx=f"g{k}")]
    layers = []
    layers += pair("inc.double_conv", "input", None, False, "mid0", "x0", 0, n_channels, None)
    for l in range(1, 5):
        layers += pair(f"down{l}.maxpool_conv.1.double_conv", f"x{l - 1}", None, True, f"mid{l}", f"x{l}", l, CHANNELS[l - 1], f"dpool{l}",
                       dskip=f"dcat{l - 1}")
    for i, l in enumerate((3, 2, 1, 0)):
        layers += pair(f"up{i + 1}.conv.double_conv", f"x{l}", f"up{l}", False, f"{decoder_mid}{l}", f"d{l}", l, 2 * CHANNELS[l], f"dcat{l}")
        layers[-2].update(up=i, up_name=f"up{i + 1}.up")
    return layers


# ---- the module: the reference's state-dict names and shapes ----------------------------------------------------------------------
def _double_conv(cin, cout):
    m = nn.Module()
    m.double_conv = nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True),
                                  nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
    return m


def _down(cin, cout):
    m = nn.Module()
    m.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), _double_conv(cin, cout))
    return m


def _up(cin, cout):
    m = nn.Module()
    m.up = nn.ConvTranspose2d(cin, cin // 2, kernel_size=2, stride=2)
    m.conv = _double_conv(cin, cout)
    return m


class RayDropUNet(nn.Module):
    """UNet(n_channels, 1, bilinear=False) of lidarnvs/unet.py for inference.  Parameters and buffers carry the reference's names
    and shapes (inc.double_conv.0.weight, ..., up1.up.weight, outc.conv.bias, num_batches_tracked included), so a checkpoint of
    the reference loads with load_state_dict and state_dict() loads into the reference's module.  The submodules only hold the
    parameters; forward() runs the fused kernels on images packed from them by pack().

    The module is built in eval mode and forward() refuses training mode: BatchNorm with batch statistics is not implemented.
    forward / predict_mask return tensors that belong to the cached workspace of their (N, H, W): the next call of that shape
    overwrites them (clone to keep one)."""

    def __init__(self, n_channels=10, n_classes=1, bilinear=False):
        super().__init__()
        if bilinear:
            raise NotImplementedError("RayDropUNet: bilinear=True (nn.Upsample) is not implemented; the reference's default "
                                      "and its checkpoints use the transposed convolution")
        if int(n_classes) != 1:
            raise NotImplementedError(f"RayDropUNet: n_classes must be 1 (a ray-drop logit), got {n_classes}")
        if not 1 <= int(n_channels) <= 32:
            raise ValueError(f"RayDropUNet: n_channels must be 1 .. 32, got {n_channels}")
        self.n_channels, self.n_classes, self.bilinear = int(n_channels), 1, False
        self._packed = None
        self._workspaces = {}
        self.inc = _double_conv(self.n_channels, 64)
        for i in range(4):
            setattr(self, f"down{i + 1}", _down(CHANNELS[i], CHANNELS[i + 1]))
        for i in range(4):
            setattr(self, f"up{i + 1}", _up(CHANNELS[4 - i], CHANNELS[3 - i]))
        self.outc = nn.Module()
        self.outc.conv = nn.Conv2d(64, 1, kernel_size=1)
        self.eval()

    @classmethod
    def from_checkpoint(cls, path, n_channels=10, device=None):
        """A module with the state dict torch.save wrote at `path` (what raydrop_train_poisson.py saves), on `device` or the
        current GPU."""
        state = torch.load(path, map_location="cpu")
        net = cls(n_channels=n_channels)
        net.load_state_dict(state)
        return net.to(torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))

    # -- packing --
    @staticmethod
    def _pack_conv(conv, bn):
        w = conv.weight.detach()
        cout, cin = w.shape[0], w.shape[1]
        cpad = (cin + 31) // 32 * 32
        img = torch.zeros(cout, 3, 3, cpad, dtype=torch.float16, device=w.device)
        img[..., :cin] = w.permute(0, 2, 3, 1).to(torch.float16)  # round to nearest even
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        t = bn.bias.detach().double() - bn.running_mean.detach().double() * s
        return img.reshape(cout, 9, cpad).contiguous(), s.to(torch.float32).contiguous(), t.to(torch.float32).contiguous()

    @torch.no_grad()
    def pack(self):
        """The fp16 weight images and fp32 scale / shift vectors the kernels read (layouts: include/lidarnerf_hip.h): one-time
        torch ops wherever the parameters live; load_state_dict and every move or cast (_apply) call it.  After changing a
        parameter in place, call it again."""
        table = layer_table(self.n_channels)
        convs = [self._pack_conv(self.get_submodule(lay["conv"]), self.get_submodule(lay["bn"])) for lay in table]
        ups = []
        for m in (self.get_submodule(lay["up_name"]) for lay in table if lay["up"] is not None):
            w = m.weight.detach()  # [Cin, Cout, 2, 2] -> [2dy + dx, Cout, Cin]
            ups.append((w.permute(2, 3, 1, 0).reshape(4, w.shape[1], w.shape[0]).to(torch.float16).contiguous(),
                        m.bias.detach().to(torch.float32).contiguous()))
        hw = self.outc.conv.weight.detach().reshape(64).to(torch.float16).contiguous()
        hb = self.outc.conv.bias.detach().reshape(1).to(torch.float32).contiguous()
        self._packed = {"convs": convs, "ups": ups, "head": (hw, hb)}
        return self._packed

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.pack()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._workspaces = {}
        self.pack()
        return out

    # -- inference --
    def _workspace(self, N, H, W, device):
        key = (N, H, W, device.index)
        ws = self._workspaces.get(key)
        if ws is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RayDropUNet: the workspace of a shape must exist before a call is captured (run it eagerly once)")
            layout, total = workspace_layout(N, H, W)
            need = int(_hip.lib().lnh_unet_workspace_size(N, H, W))
            if need == 0 or need != total:
                raise RuntimeError(f"RayDropUNet: lnh_unet_workspace_size({N}, {H}, {W}) = {need}, the layout needs {total}")
            raw = torch.empty(total, dtype=torch.uint8, device=device)
            ws = self._workspaces[key] = {"raw": raw, "views": carve(raw, layout),
                                          "logits": torch.empty(N, 1, H, W, dtype=torch.float32, device=device),
                                          "mask": torch.empty(N, 1, H, W, dtype=torch.float32, device=device)}
        return ws

    def _run(self, images, want_mask):
        if self.training:
            raise RuntimeError("RayDropUNet: training mode is not implemented (BatchNorm with batch statistics); call eval()")
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != self.n_channels:
            raise ValueError(f"RayDropUNet: images must be [N, {self.n_channels}, H, W]")
        N, _, H, W = images.shape
        if H < MIN_SIZE or W < MIN_SIZE or N < 1:
            raise ValueError(f"RayDropUNet: images of {H} x {W}; H and W must be at least {MIN_SIZE} (four halvings)")
        if not images.is_cuda:
            raise RuntimeError("RayDropUNet: images must live on the GPU (no CPU fallback)")
        _hip.require_symbols(_SYMBOLS, "the ray-drop U-Net")
        if self._packed is None:
            self.pack()
        convs, ups, (hw, hb) = self._packed["convs"], self._packed["ups"], self._packed["head"]
        if convs[0][0].device != images.device:
            raise RuntimeError(f"RayDropUNet: parameters on {convs[0][0].device}, images on {images.device}")
        images = images.detach().to(torch.float32).contiguous()
        ws = self._workspace(N, H, W, images.device)
        v = ws["views"]
        cur = unet_input(images, v["input"])
        for lay, packed in zip(layer_table(self.n_channels), convs):
            if lay["up"] is not None:  # a decoder block begins: the transposed convolution of what came before
                upconv2x2(cur, *ups[lay["up"]], v[lay["src1"]])
            cur = conv3x3(v[lay["src0"]], *packed, v[lay["out"]], src1=v.get(lay["src1"]), pool=lay["pool"])
        head(cur, hw, hb, ws["logits"], ws["mask"] if want_mask else None)
        return ws

    @torch.no_grad()
    def forward(self, images):
        """images f32 [N, n_channels, H, W] on the GPU (H, W >= 16) -> logits f32 [N, 1, H, W]."""
        return self._run(images, False)["logits"]

    @torch.no_grad()
    def predict_mask(self, images):
        """The 0 / 1 mask f32 [N, 1, H, W]: 1 where logit > 0, which is sigmoid(logit) > 0.5; 0 for a NaN logit."""
        return self._run(images, True)["mask"]
