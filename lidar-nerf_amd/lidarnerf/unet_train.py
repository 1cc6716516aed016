"""Training of the ray-drop U-Net of the mesh baselines (raydrop_train_poisson.py): what exists of it so far.
* The loss and the validation score of the reference's loop for the one-class net, as differentiable torch functions on any device
  and dtype; golden G18 pins them to the reference's own values.
* Backward kernels on tensors (csrc/unet_train.hip through the C ABI, include/lidarnerf_hip.h "U-Net training"): the max-pool
  backward with the skip add, the backward of the 1 x 1 head, the transposed convolution's weight pack, data gradient and weight / bias
  gradient.  One entry point each; they read no host memory and allocate nothing — the caller owns every buffer.  No CPU fallback.

* The training-mode convolution layer (csrc/unet_train_conv.hip, csrc/unet_train_wgrad.hip and the RAW epilogue of csrc/unet.hip):
  pack_conv3x3, conv3x3_raw (the forward convolution and, on the flipped and transposed image, the data gradient), bn_stats, bn_relu,
  bn_relu_backward, conv3x3_backward_weight.
* train_forward / train_backward: the whole net in training mode on a RayDropUNet's live parameters, and the gradient of the loss with
  respect to every activation and — with conv_weights=True — all 64 parameter tensors (without it the 46 that are no 3 x 3
  convolution weight), in one workspace that is allocated once per shape.

* The step around them (csrc/unet_train_step.hip): raydrop_unet_loss_and_grad (the loss and its cotangent in closed form),
  grad_sumsq and rmsprop_step over a device-resident table of tensors.  lidarnerf.unet_trainer.RayDropUNetTrainer owns a step;
  RayDropUNet itself keeps refusing training mode."""
import torch
import torch.nn.functional as F

from . import _hip
from . import unet as _unet
from .unet import CHANNELS, _nhwc

_SYMBOLS = ("lnh_unet_pool_backward", "lnh_unet_head_backward", "lnh_unet_head_backward_workspace_size", "lnh_unet_pack_upconv",
            "lnh_unet_upconv2x2_backward_data", "lnh_unet_upconv2x2_backward_weight", "lnh_unet_upconv2x2_backward_weight_workspace_size",
            "lnh_unet_pack_conv3x3", "lnh_unet_conv3x3_raw", "lnh_unet_bn_stats", "lnh_unet_bn_stats_workspace_size", "lnh_unet_bn_relu",
            "lnh_unet_bn_relu_backward", "lnh_unet_bn_relu_backward_workspace_size", "lnh_unet_conv3x3_backward_weight",
            "lnh_unet_conv3x3_backward_weight_workspace_size")


# ---- loss and validation score ------------------------------------------------------------------------------------------------------
def dice_coeff(input, target, reduce_batch_first=False, epsilon=1e-6):
    """Dice coefficient 2 |A B| / (|A| + |B|) of soft masks, averaged: per image of a batch [N, H, W] (or of the one mask [H, W]);
    with reduce_batch_first over the whole [N, H, W] batch as one set.  epsilon is added to numerator and denominator; a pair of
    empty sets (|A| + |B| = 0) scores 1."""
    if input.shape != target.shape:
        raise ValueError(f"dice_coeff: input {tuple(input.shape)} and target {tuple(target.shape)} differ")
    if reduce_batch_first and input.dim() != 3:
        raise ValueError(f"dice_coeff: reduce_batch_first needs a [N, H, W] batch, got {tuple(input.shape)}")
    keep = 0 if reduce_batch_first else max(input.dim() - 2, 0)  # leading dimensions that stay separate sets
    a, b = input.flatten(keep), target.flatten(keep)
    overlap = torch.sum(a * b, dim=-1)
    size = torch.sum(a + b, dim=-1)
    score = (2 * overlap + epsilon) / (size + epsilon)
    score = score.masked_fill(size == 0, 1.0)  # (2 . 0 + eps) / (0 + eps)
    return score.mean()


def dice_loss(input, target):
    """1 - dice_coeff over the whole batch (reduce_batch_first=True), as the reference's training loss uses it."""
    return 1 - dice_coeff(input, target, reduce_batch_first=True)


def _pair(logits, masks):
    if logits.dim() == 4 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    if logits.dim() != 3:
        raise ValueError(f"logits must be [N, 1, H, W] or [N, H, W], got {tuple(logits.shape)}")
    if masks.numel() != logits.numel():
        raise ValueError(f"masks of {tuple(masks.shape)} do not fit logits of {tuple(logits.shape)}")
    return logits, masks.reshape(logits.shape).to(logits.dtype)


def raydrop_unet_loss(logits, masks):
    """The training loss of raydrop_train_poisson.py for the one-class net: BCEWithLogitsLoss (mean) + dice_loss(sigmoid(logits),
    masks).  logits [N, 1, H, W] (or [N, H, W]), masks of as many elements holding 0 / 1 in any dtype."""
    logits, masks = _pair(logits, masks)
    return F.binary_cross_entropy_with_logits(logits, masks) + dice_loss(torch.sigmoid(logits), masks)


def raydrop_unet_dice_score(logits, masks):
    """The validation score of the reference's evaluate(): dice_coeff of the thresholded prediction sigmoid(logits) > 0.5 against
    the masks, averaged per image (reduce_batch_first=False)."""
    logits, masks = _pair(logits, masks)
    return dice_coeff((torch.sigmoid(logits) > 0.5).to(logits.dtype), masks, reduce_batch_first=False)


# ---- backward kernels on tensors ---------------------------------------------------------------------------------------------------
def pool_backward(x, dpool, dx, dskip=None):
    """lnh_unet_pool_backward: dx [N, H0, W0, C] = the gradient of MaxPool2d(2) at x for dpool [N, H0 // 2, W0 // 2, C] (to the first
    maximum of each window) + channels [0, C) of dskip [N, H0, W0, Cs] (Cs >= C), rounded once.  All fp16 NHWC."""
    N, H0, W0, C = _nhwc(x, "x").shape
    if tuple(_nhwc(dx, "dx").shape) != (N, H0, W0, C) or tuple(_nhwc(dpool, "dpool").shape) != (N, H0 // 2, W0 // 2, C):
        raise RuntimeError("lidarnerf.unet_train.pool_backward: x / dx [N, H0, W0, C], dpool [N, H0 // 2, W0 // 2, C]")
    stride = 0
    if dskip is not None:
        stride = _nhwc(dskip, "dskip").shape[3]
        if tuple(dskip.shape[:3]) != (N, H0, W0) or stride < C:
            raise RuntimeError("lidarnerf.unet_train.pool_backward: dskip must be [N, H0, W0, Cs] with Cs >= C")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_pool_backward", _hip.ptr(x), N, H0, W0, C, _hip.ptr(dpool), _hip.ptr(dskip), stride, _hip.ptr(dx))
    return dx


def head_backward_workspace_bytes(N, H, W):
    """Bytes of head_backward's workspace: 65 f32 partials per 64 pixels.  Equals lnh_unet_head_backward_workspace_size."""
    return (N * H * W + 63) // 64 * 65 * 4


def head_backward(a, weight, dlogits, ws, dx, dweight, dbias):
    """lnh_unet_head_backward: a fp16 [N, H, W, 64], weight fp16 [64], dlogits f32 [N, 1, H, W] -> dx fp16 [N, H, W, 64], dweight f32
    [64] (any shape of 64 elements, e.g. the parameter's [1, 64, 1, 1]), dbias f32 [1]."""
    N, H, W, C = _nhwc(a, "a").shape
    if C != 64 or tuple(_nhwc(dx, "dx").shape) != (N, H, W, 64) or weight.dtype != torch.float16 or weight.numel() != 64:
        raise RuntimeError("lidarnerf.unet_train.head_backward: a / dx fp16 [N, H, W, 64], weight fp16 [64]")
    for t, n, what in ((dlogits, N * H * W, "dlogits"), (dweight, 64, "dweight"), (dbias, 1, "dbias")):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == n):
            raise RuntimeError(f"lidarnerf.unet_train.head_backward: {what} must be f32 with {n} elements")
    _hip.require_cuda(weight, dlogits, dweight, dbias)
    have = _ws_bytes(ws, head_backward_workspace_bytes(N, H, W), "head_backward")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_head_backward", _hip.ptr(a), N, H, W, _hip.ptr(weight), _hip.ptr(dlogits), _hip.ptr(ws), have, _hip.ptr(dx),
              _hip.ptr(dweight), _hip.ptr(dbias))
    return dx, dweight, dbias


def pack_upconv(weight, fwd, bwd=None):
    """lnh_unet_pack_upconv: weight f32 [Cin, Cout, 2, 2] (the parameter) -> fwd fp16 [4, Cout, Cin] (what lidarnerf.unet.upconv2x2
    reads) and, if given, bwd fp16 [Cin, 4, Cout] (what upconv2x2_backward_data reads)."""
    if not (torch.is_tensor(weight) and weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4 and
            weight.is_contiguous() and tuple(weight.shape[2:]) == (2, 2)):
        raise RuntimeError("lidarnerf.unet_train.pack_upconv: weight must be a contiguous f32 [Cin, Cout, 2, 2] GPU tensor")
    Cin, Cout = weight.shape[:2]
    for t, shape, what in ((fwd, (4, Cout, Cin), "fwd"), (bwd, (Cin, 4, Cout), "bwd")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError(f"lidarnerf.unet_train.pack_upconv: {what} must be contiguous fp16 {shape} on the GPU")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_pack_upconv", _hip.ptr(weight.detach()), Cin, Cout, _hip.ptr(fwd), _hip.ptr(bwd))
    return fwd, bwd


def upconv2x2_backward_data(dy, weight, dx, offset=0):
    """lnh_unet_upconv2x2_backward_data: dx fp16 [N, H, W, Cin] from channels [offset, offset + Cout) of dy fp16 [N, Hd, Wd, Cs] (Hd,
    Wd = 2H, 2W or one larger: the concatenation's gradient, read in place) and weight fp16 [Cin, 4, Cout] (pack_upconv's bwd)."""
    N, H, W, Cin = _nhwc(dx, "dx").shape
    Nd, Hd, Wd, Cs = _nhwc(dy, "dy").shape
    if weight.dtype != torch.float16 or weight.dim() != 3 or weight.shape[0] != Cin or weight.shape[1] != 4 or Nd != N:
        raise RuntimeError("lidarnerf.unet_train.upconv2x2_backward_data: weight fp16 [Cin, 4, Cout], dy / dx of the same batch")
    _hip.require_cuda(weight)
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_upconv2x2_backward_data", _hip.ptr(dy), Hd, Wd, Cs, int(offset), N, H, W, Cin, weight.shape[2], _hip.ptr(weight),
              _hip.ptr(dx))
    return dx


def upconv_wgrad_slices(M, Cin, Cout):
    """(S, L): the slices upconv2x2_backward_weight cuts M input pixels into and the pixels per slice, from the shape alone."""
    S = min((M + 255) // 256, max(1, (16 << 20) // (16 * Cin * Cout)))
    L = ((M + S - 1) // S + 31) // 32 * 32
    return (M + L - 1) // L, L


def upconv2x2_backward_weight_workspace_bytes(N, H, W, Cin, Cout):
    """Bytes of upconv2x2_backward_weight's workspace: S slices of 4 Cin Cout + Cout f32.  Equals the C size function."""
    return upconv_wgrad_slices(N * H * W, Cin, Cout)[0] * (4 * Cin * Cout + Cout) * 4


def upconv2x2_backward_weight(x, dy, ws, dweight, dbias, offset=0):
    """lnh_unet_upconv2x2_backward_weight: dweight f32 [Cin, Cout, 2, 2] and dbias f32 [Cout] of the transposed convolution from its
    input x fp16 [N, H, W, Cin] and channels [offset, offset + Cout) of dy fp16 [N, Hd, Wd, Cs], read in place."""
    N, H, W, Cin = _nhwc(x, "x").shape
    Nd, Hd, Wd, Cs = _nhwc(dy, "dy").shape
    if not (torch.is_tensor(dweight) and dweight.dtype == torch.float32 and dweight.dim() == 4 and dweight.is_contiguous() and
            dweight.shape[0] == Cin and tuple(dweight.shape[2:]) == (2, 2)) or Nd != N:
        raise RuntimeError("lidarnerf.unet_train.upconv2x2_backward_weight: dweight contiguous f32 [Cin, Cout, 2, 2], x / dy of one batch")
    Cout = dweight.shape[1]
    if not (torch.is_tensor(dbias) and dbias.dtype == torch.float32 and dbias.numel() == Cout and dbias.is_contiguous()):
        raise RuntimeError(f"lidarnerf.unet_train.upconv2x2_backward_weight: dbias must be contiguous f32 [{Cout}]")
    _hip.require_cuda(dweight, dbias)
    have = _ws_bytes(ws, upconv2x2_backward_weight_workspace_bytes(N, H, W, Cin, Cout), "upconv2x2_backward_weight")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_upconv2x2_backward_weight", _hip.ptr(x), _hip.ptr(dy), Hd, Wd, Cs, int(offset), N, H, W, Cin, Cout, _hip.ptr(ws),
              have, _hip.ptr(dweight), _hip.ptr(dbias))
    return dweight, dbias


# ---- the training-mode convolution layer -------------------------------------------------------------------------------------------
def pack_conv3x3(weight, fwd, bwd=None):
    """lnh_unet_pack_conv3x3: weight f32 [Cout, Cin, 3, 3] (the parameter) -> fwd fp16 [Cout, 9, Cpad] (what conv3x3 / conv3x3_raw read;
    Cpad = 32 for Cin <= 32, else Cin) and, if given, bwd fp16 [Cin, 9, Cout] with bwd[ci, t, co] = weight[co, ci, 8 - t] (what
    conv3x3_raw reads as the data gradient; Cin a multiple of 64)."""
    if not (torch.is_tensor(weight) and weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4 and
            weight.is_contiguous() and tuple(weight.shape[2:]) == (3, 3)):
        raise RuntimeError("lidarnerf.unet_train.pack_conv3x3: weight must be a contiguous f32 [Cout, Cin, 3, 3] GPU tensor")
    Cout, Cin = weight.shape[:2]
    cpad = 32 if Cin <= 32 else Cin
    for t, shape, what in ((fwd, (Cout, 9, cpad), "fwd"), (bwd, (Cin, 9, Cout), "bwd")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous() and tuple(t.shape) == shape):
            raise RuntimeError(f"lidarnerf.unet_train.pack_conv3x3: {what} must be contiguous fp16 {shape} on the GPU")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_pack_conv3x3", _hip.ptr(weight.detach()), Cout, Cin, _hip.ptr(fwd), _hip.ptr(bwd))
    return fwd, bwd


def conv3x3_raw(src0, weight, out, src1=None, pool=False, tile=0):
    """lnh_unet_conv3x3_raw: lidarnerf.unet.conv3x3 without scale / shift, out = fp16(acc).  With pack_conv3x3's bwd image as weight and
    dz as src0 it is the data gradient of the layer: out [N, H, W, C0 + C1]."""
    operand, N, Cout, fits = _unet.conv_operand(src0, src1, pool, out, "out")
    if not fits or not torch.is_tensor(weight) or tuple(weight.shape) != (Cout, 9, operand[1] + operand[6]) or weight.dtype != torch.float16:
        raise RuntimeError("lidarnerf.unet_train.conv3x3_raw: shapes of out / weight do not fit the sources")
    _hip.require_cuda(weight)
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_conv3x3_raw", *operand, _hip.ptr(weight), N, Cout, int(tile), _hip.ptr(out))
    return out


def bn_partials(M):
    """(P, parts): the pixels per partial of bn_stats / bn_relu_backward and their number, from the shape alone."""
    P = 256 * ((M + (1 << 14) - 1) >> 14)
    return P, (M + P - 1) // P


def bn_stats_workspace_bytes(M, C):
    """Bytes of bn_stats' (and bn_relu_backward's) workspace: 2 C float64 per partial.  Equals the C size functions."""
    return bn_partials(M)[1] * 2 * C * 8


bn_relu_backward_workspace_bytes = bn_stats_workspace_bytes


def _vec(t, C, what, where):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == C and t.is_contiguous()):
        raise RuntimeError(f"lidarnerf.unet_train.{where}: {what} must be contiguous f32 [{C}]")
    return t


def _ws_bytes(ws, need, where):
    _hip.require_cuda(ws)
    have = ws.numel() * ws.element_size()
    if have < need:
        raise RuntimeError(f"lidarnerf.unet_train.{where}: the workspace holds {have} bytes, {need} needed")
    return have


def bn_stats(z, gamma, beta, eps, momentum, ws, mean, invstd, scale, shift, running_mean=None, running_var=None):
    """lnh_unet_bn_stats: z fp16 [N, H, W, C] (M = N H W >= 2 values per channel) -> mean, invstd, scale = gamma invstd, shift = beta -
    mean scale, all f32 [C], and the in-place update of running_mean / running_var (f32 [C]) where given."""
    N, H, W, C = _nhwc(z, "z").shape
    M = N * H * W
    if M < 2:
        raise ValueError("lidarnerf.unet_train.bn_stats: expected more than 1 value per channel when training")
    for t, what in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (invstd, "invstd"), (scale, "scale"), (shift, "shift")):
        _vec(t, C, what, "bn_stats")
    for t, what in ((running_mean, "running_mean"), (running_var, "running_var")):
        if t is not None:
            _vec(t, C, what, "bn_stats")
    _hip.require_cuda(gamma, beta, mean, invstd, scale, shift, running_mean, running_var)
    have = _ws_bytes(ws, bn_stats_workspace_bytes(M, C), "bn_stats")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_bn_stats", _hip.ptr(z), M, C, _hip.ptr(gamma), _hip.ptr(beta), float(eps), float(momentum), _hip.ptr(ws), have,
              _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(scale), _hip.ptr(shift), _hip.ptr(running_mean), _hip.ptr(running_var))
    return mean, invstd, scale, shift


def bn_relu(z, scale, shift, a):
    """lnh_unet_bn_relu: a = fp16(max(fmaf(float(z), scale, shift), 0)), z / a fp16 [N, H, W, C], scale / shift f32 [C]."""
    N, H, W, C = _nhwc(z, "z").shape
    if tuple(_nhwc(a, "a").shape) != (N, H, W, C):
        raise RuntimeError("lidarnerf.unet_train.bn_relu: z and a must have one shape")
    _hip.require_cuda(_vec(scale, C, "scale", "bn_relu"), _vec(shift, C, "shift", "bn_relu"))
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_bn_relu", _hip.ptr(z), N * H * W, C, _hip.ptr(scale), _hip.ptr(shift), _hip.ptr(a))
    return a


def bn_relu_backward(z, a, da, mean, invstd, scale, ws, dz, dgamma, dbeta):
    """lnh_unet_bn_relu_backward: from the layer's stored z and a, bn_stats' mean / invstd / scale and the cotangent da -> dgamma, dbeta
    f32 [C] and dz fp16 [N, H, W, C] (dz may be da)."""
    N, H, W, C = _nhwc(z, "z").shape
    M = N * H * W
    if M < 2:
        raise ValueError("lidarnerf.unet_train.bn_relu_backward: expected more than 1 value per channel")
    for t, what in ((a, "a"), (da, "da"), (dz, "dz")):
        if tuple(_nhwc(t, what).shape) != (N, H, W, C):
            raise RuntimeError("lidarnerf.unet_train.bn_relu_backward: z, a, da and dz must have one shape")
    for t, what in ((mean, "mean"), (invstd, "invstd"), (scale, "scale"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _vec(t, C, what, "bn_relu_backward")
    _hip.require_cuda(mean, invstd, scale, dgamma, dbeta)
    have = _ws_bytes(ws, bn_relu_backward_workspace_bytes(M, C), "bn_relu_backward")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_bn_relu_backward", _hip.ptr(z), _hip.ptr(a), _hip.ptr(da), M, C, _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(scale),
              _hip.ptr(ws), have, _hip.ptr(dz), _hip.ptr(dgamma), _hip.ptr(dbeta))
    return dz, dgamma, dbeta


def conv_wgrad_slices(M, Cp, Cout):
    """(S, L): the slices conv3x3_backward_weight cuts M output pixels into and the pixels per slice, from the shape alone (Cp = C0 +
    C1 as stored: 32 for the first layer)."""
    S = min((M + 255) // 256, max(1, (32 << 20) // (36 * Cp * Cout)))
    L = ((M + S - 1) // S + 31) // 32 * 32
    return (M + L - 1) // L, L


def conv3x3_backward_weight_workspace_bytes(N, H0, W0, pool, C0, C1, Cout):
    """Bytes of conv3x3_backward_weight's workspace: S slices of [9, Cout, C0 + C1] f32; 0 for a shape the kernel refuses.  Equals
    lnh_unet_conv3x3_backward_weight_workspace_size."""
    H, W = (H0 // 2, W0 // 2) if pool else (H0, W0)
    c_ok = (C0 == 32 and C1 == 0) or (64 <= C0 <= 1024 and C0 % 64 == 0 and C1 in (0, C0))
    if not (pool in (0, 1, False, True) and N >= 1 and H >= 1 and W >= 1 and N * H0 * W0 <= 1 << 26 and c_ok and
            64 <= Cout <= 1024 and Cout % 64 == 0):
        return 0
    return conv_wgrad_slices(N * H * W, C0 + C1, Cout)[0] * 36 * (C0 + C1) * Cout


def conv3x3_backward_weight(src0, dz, ws, dweight, src1=None, pool=False, variant=0):
    """lnh_unet_conv3x3_backward_weight: dweight f32 [Cout, Cin, 3, 3] (the parameter's layout, overwritten) = the gradient of the
    layer's weight for dz fp16 [N, H, W, Cout], from the operand the forward convolution read: src0 fp16 [N, H0, W0, C0] (pooled 2 x 2
    on read with pool), then the channels of src1 fp16 [N, H1, W1, C1].  Cin = C0 + C1, or the real channel count (up to 32) of the
    padded first layer.  variant: 0, _hip.UNET_WGRAD_GATHER or _hip.UNET_WGRAD_TR (the same bits)."""
    operand, N, Cout, fits = _unet.conv_operand(src0, src1, pool, dz, "dz")
    if not (torch.is_tensor(dweight) and dweight.dtype == torch.float32 and dweight.dim() == 4 and dweight.is_contiguous() and
            dweight.shape[0] == Cout and tuple(dweight.shape[2:]) == (3, 3)) or not fits:
        raise RuntimeError("lidarnerf.unet_train.conv3x3_backward_weight: dweight contiguous f32 [Cout, Cin, 3, 3], dz [N, H, W, Cout] "
                           "over the sources' batch and output size")
    _hip.require_cuda(dweight)
    _, C0, H0, W0, _, _, C1, _, _ = operand  # (a shape the kernel refuses needs 0 bytes here: the entry point names the fault)
    have = _ws_bytes(ws, conv3x3_backward_weight_workspace_bytes(N, H0, W0, pool, C0, C1, Cout), "conv3x3_backward_weight")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_conv3x3_backward_weight", *operand, _hip.ptr(dz), N, Cout, dweight.shape[1], int(variant), _hip.ptr(ws), have,
              _hip.ptr(dweight))
    return dweight


# ---- the whole net in training mode ---------------------------------------------------------------------------------------------------
def train_layers(n_channels=10):
    """lidarnerf.unet.layer_table with the buffer names of training: the decoder's first activations are dmid{l}."""
    return _unet.layer_table(n_channels, decoder_mid="dmid")


def train_workspace_layout(N, H, W, n_channels=10):
    """([(name, byte offset, shape, dtype)], total bytes) of everything train_forward / train_backward touch, every buffer 256-byte
    aligned: the inference layout of lidarnerf.unet.workspace_layout at its offsets, then
      dmid{l}            the decoder's first activation, l = 0 .. 3 (inference reuses mid{l}; the backward needs both)
      z{k}, g{k}         the raw convolution output of layer k = 0 .. 17 and the gradient buffer of its shape: da, then in place dz
      dcat{l}, dpool{l}  the data gradient of a concatenating layer [N, h, w, 2 C] and of a pooling layer (the pooled tensor's)
      stat{k}            f32 [6, C]: mean, invstd, scale, shift, dgamma, dbeta
      wf{k}, wb{k}       the packed forward and (k >= 1) data-gradient weight images; uf{i}, ub{i}, hw: the transposed convolutions', the head's
      dupw{i}, dupb{i}, dhw, dhb   f32 parameter gradients of the transposed convolutions and the head
      ws_bn, ws_head, ws_up        the partials workspaces (each the largest any layer needs)
      logits             f32 [N, 1, H, W]
      dcw{k}             f32 [Cout, Cin, 3, 3]: the weight gradient of convolution k, the parameter's shape
      ws_cw              conv3x3_backward_weight's partials, as large as the largest layer needs."""
    sizes = _unet.level_sizes(H, W)
    f16, f32, u8 = torch.float16, torch.float32, torch.uint8
    bufs = [(name, shape, f16) for name, _, shape in _unet.workspace_layout(N, H, W)[0]]
    bufs += [(f"dmid{l}", (N,) + sizes[l] + (CHANNELS[l],), f16) for l in range(4)]
    layers = train_layers(n_channels)
    for k, lay in enumerate(layers):
        shape = (N,) + sizes[lay["level"]] + (lay["cout"],)
        bufs += [(f"z{k}", shape, f16), (f"g{k}", shape, f16)]
    for l in range(4):
        bufs.append((f"dcat{l}", (N,) + sizes[l] + (2 * CHANNELS[l],), f16))
    for l in range(1, 5):
        bufs.append((f"dpool{l}", (N,) + sizes[l] + (CHANNELS[l - 1],), f16))
    for k, lay in enumerate(layers):
        bufs.append((f"stat{k}", (6, lay["cout"]), f32))
    for k, lay in enumerate(layers):
        cin = lay["cin"]
        bufs.append((f"wf{k}", (lay["cout"], 9, 32 if cin <= 32 else cin), f16))
        if k:
            bufs.append((f"wb{k}", (cin, 9, lay["cout"]), f16))
    for i in range(4):
        cin = CHANNELS[4 - i]
        bufs += [(f"uf{i}", (4, cin // 2, cin), f16), (f"ub{i}", (cin, 4, cin // 2), f16), (f"dupw{i}", (cin, cin // 2, 2, 2), f32),
                 (f"dupb{i}", (cin // 2,), f32)]
    bufs += [("hw", (64,), f16), ("dhw", (1, 64, 1, 1), f32), ("dhb", (1,), f32)]
    ws_bn = max(bn_stats_workspace_bytes(N * sizes[lay["level"]][0] * sizes[lay["level"]][1], lay["cout"]) for lay in layers)
    ws_up = max(upconv2x2_backward_weight_workspace_bytes(N, sizes[l + 1][0], sizes[l + 1][1], CHANNELS[l + 1], CHANNELS[l]) for l in range(4))
    bufs += [("ws_bn", (ws_bn,), u8), ("ws_head", (head_backward_workspace_bytes(N, H, W),), u8), ("ws_up", (ws_up,), u8),
             ("logits", (N, 1, H, W), f32)]
    bufs += [(f"dcw{k}", (lay["cout"], lay["cin"], 3, 3), f32) for k, lay in enumerate(layers)]
    bufs.append(("ws_cw", (max(_conv_wgrad_bytes(N, sizes, lay) for lay in layers),), u8))
    return _unet.place(bufs)


def _conv_wgrad_bytes(N, sizes, lay):
    """The weight-gradient workspace of one entry of train_layers at level sizes `sizes`."""
    l = lay["level"]
    h0, w0 = sizes[l - 1] if lay["pool"] else sizes[l]
    c0 = max(32, lay["cin"]) if lay["src1"] is None else lay["cin"] // 2
    return conv3x3_backward_weight_workspace_bytes(N, h0, w0, lay["pool"], c0, lay["cin"] - c0 if lay["src1"] is not None else 0, lay["cout"])


def _train_state(net, N, H, W, device):
    key = (N, H, W, device.index, net.n_channels)
    cache = net.__dict__.setdefault("_train_states", {})
    st = cache.get(key)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lidarnerf.unet_train: the workspace of a shape must exist before a call is captured (run it eagerly once)")
        layout, total = train_workspace_layout(N, H, W, net.n_channels)
        raw = torch.empty(total, dtype=torch.uint8, device=device)
        views = _unet.carve(raw, layout)
        layers = train_layers(net.n_channels)
        grads = {"outc.conv.weight": views["dhw"], "outc.conv.bias": views["dhb"]}
        conv_grads = {}
        for k, lay in enumerate(layers):
            conv_grads[lay["conv"] + ".weight"] = views[f"dcw{k}"]
            s = views[f"stat{k}"]
            lay.update(index=k, operand=(views[lay["src0"]], views.get(lay["src1"])), z=views[f"z{k}"], a=views[lay["out"]], dz=views[f"g{k}"],
                       dweight=views[f"dcw{k}"], mean=s[0], invstd=s[1], scale=s[2], shift=s[3], dgamma=s[4], dbeta=s[5])
            grads[lay["bn"] + ".weight"], grads[lay["bn"] + ".bias"] = s[4], s[5]
        for name, i in ((lay["up_name"], lay["up"]) for lay in layers if lay["up"] is not None):
            grads[name + ".weight"], grads[name + ".bias"] = views[f"dupw{i}"], views[f"dupb{i}"]
        # "grads": all 64 names; "grads_no_conv": the 46 a train_backward without the convolution weights fills and returns
        st = cache[key] = {"key": key, "raw": raw, "views": views, "layers": layers, "grads": {**grads, **conv_grads},
                           "grads_no_conv": grads, "logits": views["logits"]}
    return st


def _live(t, what):
    t = t.detach()
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"lidarnerf.unet_train: {what} must be a contiguous f32 GPU tensor (the live parameter is read on the device)")
    return t


def train_forward(net, images, state=None):
    """The forward of the net in training mode (BatchNorm on the batch's statistics), whatever mode `net` is in: images f32
    [N, n_channels, H, W] on the GPU -> (logits f32 [N, 1, H, W], state).  `net` is a lidarnerf.unet.RayDropUNet; its fp32 parameters
    are read live and packed on the device, its running_mean / running_var / num_batches_tracked are updated in place as torch's
    BatchNorm2d does, and its cached inference pack is dropped (the next inference call packs again, from the new statistics).
    The chain: input pack; per layer pack_conv3x3 -> conv3x3_raw -> bn_stats -> bn_relu; lidarnerf.unet's upconv2x2 and head.

    `state` (None: the net's cached state of this shape, made at the first call) owns every buffer — train_workspace_layout — and
    the returned logits: the next call of the shape overwrites them.  After the first call of a shape nothing is allocated and
    nothing waits for the device; a call can be captured in a graph."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != net.n_channels:
        raise ValueError(f"lidarnerf.unet_train.train_forward: images must be [N, {net.n_channels}, H, W]")
    N, _, H, W = images.shape
    if H < _unet.MIN_SIZE or W < _unet.MIN_SIZE or N < 1:
        raise ValueError(f"lidarnerf.unet_train.train_forward: images of {H} x {W}; H and W must be at least {_unet.MIN_SIZE}")
    if not images.is_cuda:
        raise RuntimeError("lidarnerf.unet_train.train_forward: images must live on the GPU (no CPU fallback)")
    _hip.require_symbols(_unet._SYMBOLS + _SYMBOLS, "U-Net training")
    if state is None:
        state = _train_state(net, N, H, W, images.device)
    elif state["key"] != (N, H, W, images.device.index, net.n_channels):
        raise RuntimeError(f"lidarnerf.unet_train.train_forward: the state belongs to {state['key']}, not to these images")
    v = state["views"]
    _unet.unet_input(images.detach().to(torch.float32).contiguous(), v["input"])
    counters = []
    cur = None
    for k, lay in enumerate(state["layers"]):
        if lay["up"] is not None:  # a decoder block begins: the transposed convolution of what came before
            i, up = lay["up"], net.get_submodule(lay["up_name"])
            pack_upconv(_live(up.weight, "up.weight"), v[f"uf{i}"], v[f"ub{i}"])
            _unet.upconv2x2(cur, v[f"uf{i}"], _live(up.bias, "up.bias"), v[lay["src1"]])
        conv, bn = net.get_submodule(lay["conv"]), net.get_submodule(lay["bn"])
        if bn.momentum is None:
            raise NotImplementedError("lidarnerf.unet_train.train_forward: BatchNorm with momentum=None (cumulative average)")
        pack_conv3x3(_live(conv.weight, "conv.weight"), v[f"wf{k}"], v.get(f"wb{k}"))
        src0, src1 = lay["operand"]
        conv3x3_raw(src0, v[f"wf{k}"], lay["z"], src1=src1, pool=lay["pool"])
        bn_stats(lay["z"], _live(bn.weight, "bn.weight"), _live(bn.bias, "bn.bias"), bn.eps, bn.momentum, v["ws_bn"], lay["mean"],
                 lay["invstd"], lay["scale"], lay["shift"], bn.running_mean, bn.running_var)
        cur = bn_relu(lay["z"], lay["scale"], lay["shift"], lay["a"])
        counters.append(bn.num_batches_tracked)
    v["hw"].copy_(net.outc.conv.weight.detach().reshape(64))
    _unet.head(cur, v["hw"], _live(net.outc.conv.bias, "outc.conv.bias"), state["logits"])
    torch._foreach_add_(counters, 1)
    net._packed = None  # (as load_state_dict: the inference images no longer match the buffers)
    return state["logits"], state


def train_backward(net, state, dlogits, conv_weights=False):
    """The backward of train_forward's last call on `state` for the cotangent dlogits f32 [N, 1, H, W], used as given (loss scaling is
    the caller's; everything here is linear in it): {state-dict name: f32 gradient} for the 36 BatchNorm weights / biases, the 8
    transposed-convolution tensors and the 2 head tensors.  Without conv_weights the weights of the 18 3 x 3 convolutions are ABSENT
    from the dict and their kernel is not launched; with conv_weights=True each layer's conv3x3_backward_weight is launched once its
    dz exists — from state["layers"][k]'s `operand` (src0, src1; `pool` says whether src0 is pooled on read) and `dz` — and the dict
    holds all 64 names, the other 46 with the same bits.  The chain, in the order of the float64 restatement: head_backward; per
    layer bn_relu_backward, the weight gradient and the raw convolution on the flipped image; pool_backward with the skip gradient;
    upconv2x2_backward_weight / _data reading the concatenating layer's gradient in place.  The returned tensors belong to `state`;
    nothing is allocated, nothing waits."""
    v, layers = state["views"], state["layers"]
    N, H, W = state["key"][:3]
    if not (torch.is_tensor(dlogits) and dlogits.is_cuda and dlogits.dtype == torch.float32 and dlogits.is_contiguous() and
            tuple(dlogits.shape) == (N, 1, H, W)):
        raise RuntimeError(f"lidarnerf.unet_train.train_backward: dlogits must be a contiguous f32 [{N}, 1, {H}, {W}] GPU tensor")
    grads = state["grads"] if conv_weights else state["grads_no_conv"]
    head_backward(layers[-1]["a"], v["hw"], dlogits.detach(), v["ws_head"], layers[-1]["dz"], grads["outc.conv.weight"],
                  grads["outc.conv.bias"])
    for k in range(len(layers) - 1, -1, -1):
        lay, before = layers[k], layers[k - 1]  # (`before` is read only where a layer has one: up, pool)
        dx = v.get(lay["dx"])
        bn_relu_backward(lay["z"], lay["a"], lay["dz"], lay["mean"], lay["invstd"], lay["scale"], v["ws_bn"], lay["dz"], lay["dgamma"],
                         lay["dbeta"])
        if conv_weights:
            conv3x3_backward_weight(lay["operand"][0], lay["dz"], v["ws_cw"], lay["dweight"], src1=lay["operand"][1], pool=lay["pool"])
        if dx is not None:
            conv3x3_raw(lay["dz"], v[f"wb{k}"], dx)
        if lay["up"] is not None:  # dx is the concatenation's gradient: its second half is the transposed convolution's, read in place
            i, half = lay["up"], lay["cin"] // 2
            upconv2x2_backward_weight(before["a"], dx, v["ws_up"], v[f"dupw{i}"], v[f"dupb{i}"], offset=half)
            upconv2x2_backward_data(dx, v[f"ub{i}"], before["dz"], offset=half)
        if lay["pool"]:
            pool_backward(lay["operand"][0], dx, before["dz"], dskip=v[lay["dskip"]])
    return grads


# ---- the step around forward and backward: loss cotangent, sum of squares, clip + RMSprop (csrc/unet_train_step.hip) -------------------
def loss_grad_partials(M):
    """(E, parts): the elements per workgroup of raydrop_unet_loss_and_grad and the number of float64 partials, from M alone."""
    E = 256 * ((M + (1 << 16) - 1) >> 16)
    return E, (M + E - 1) // E


def loss_grad_workspace_bytes(M):
    """Bytes of raydrop_unet_loss_and_grad's workspace: three float64 per partial; 0 for an M the kernel refuses.  Equals
    lnh_unet_loss_grad_workspace_size."""
    return loss_grad_partials(M)[1] * 24 if 1 <= M <= 1 << 26 else 0


def raydrop_unet_loss_and_grad(logits, masks, dlogits, loss, ws, loss_scale=1.0):
    """lnh_unet_loss_grad: raydrop_unet_loss and its gradient in closed form, no autograd.  logits f32 [N, 1, H, W] (any shape of M
    elements), masks of M elements holding 0 / 1 as f32, uint8 or bool -> loss f32 [1] and dlogits f32 (M elements) = loss_scale
    dL/dlogits.  Every element is formed in float64 from fixed-order float64 sums and rounded once."""
    for t, what in ((logits, "logits"), (dlogits, "dlogits"), (loss, "loss")):
        if not (torch.is_tensor(t) and t.dtype == torch.float32):
            raise RuntimeError(f"lidarnerf.unet_train.raydrop_unet_loss_and_grad: {what} must be an f32 tensor")
    M = logits.numel()
    if not torch.is_tensor(masks) or masks.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise RuntimeError("lidarnerf.unet_train.raydrop_unet_loss_and_grad: masks must be f32, uint8 or bool")
    if masks.numel() != M or dlogits.numel() != M or loss.numel() != 1:
        raise RuntimeError(f"lidarnerf.unet_train.raydrop_unet_loss_and_grad: masks and dlogits must have the logits' {M} elements, loss one")
    _hip.require_cuda(logits, masks, dlogits, loss, ws)
    have = ws.numel() * ws.element_size()
    _hip.require_symbols(_STEP_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_loss_grad", _hip.ptr(logits.detach()), _hip.ptr(masks), _hip.UNET_MASK_F32 if masks.dtype == torch.float32 else
              _hip.UNET_MASK_U8, M, float(loss_scale), _hip.ptr(ws), have, _hip.ptr(loss), _hip.ptr(dlogits))
    return loss, dlogits


_STEP_SYMBOLS = ("lnh_unet_loss_grad", "lnh_unet_loss_grad_workspace_size", "lnh_unet_grad_sumsq", "lnh_unet_grad_sumsq_workspace_size",
                 "lnh_unet_rmsprop_step")
GRAD_SUMSQ_BLOCKS = 1024


def grad_sumsq_workspace_bytes():
    """Bytes of grad_sumsq's workspace: one float64 per workgroup.  Equals lnh_unet_grad_sumsq_workspace_size."""
    return GRAD_SUMSQ_BLOCKS * 8


def step_table(params, grads, square_avgs, momentum_buffers=None):
    """The device-resident table grad_sumsq and rmsprop_step read: int64 [n, 5] of (param, grad, square_avg, momentum_buffer
    pointers, element count), one row per tensor (lnh_urs_tensor).  Contiguous f32 GPU tensors of equal sizes; the table holds
    addresses only, the caller keeps the tensors alive.  momentum_buffers None: NULL pointers, for momentum = 0; the returned tensor
    carries `has_momentum_buffers`, the host-side note by which rmsprop_step refuses momentum > 0 on such a table (the entry point
    cannot see into a device-resident table)."""
    n = len(params)
    if not 1 <= n <= _hip.URS_MAX_TENSORS or len(grads) != n or len(square_avgs) != n or (momentum_buffers is not None and len(momentum_buffers) != n):
        raise RuntimeError(f"lidarnerf.unet_train.step_table: 1 .. {_hip.URS_MAX_TENSORS} tensors, as many of each kind")
    rows = []
    for k in range(n):
        group = [params[k], grads[k], square_avgs[k]] + ([] if momentum_buffers is None else [momentum_buffers[k]])
        for t in group:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == params[k].numel()):
                raise RuntimeError(f"lidarnerf.unet_train.step_table: tensor {k}: contiguous f32 GPU tensors of one size")
        rows.append([t.data_ptr() for t in group] + ([0] if momentum_buffers is None else []) + [params[k].numel()])
    table = torch.tensor(rows, dtype=torch.int64, device=params[0].device)
    table.has_momentum_buffers = momentum_buffers is not None
    return table


def _table_state(table, n_tensors, state, where):
    if not (torch.is_tensor(table) and table.dtype == torch.int64 and table.is_contiguous() and table.numel() >= _hip.URS_TENSOR_WORDS * max(int(n_tensors), 0)):
        raise RuntimeError(f"lidarnerf.unet_train.{where}: the table must be a contiguous int64 [n_tensors, {_hip.URS_TENSOR_WORDS}] tensor")
    if not (torch.is_tensor(state) and state.dtype == torch.float64 and state.is_contiguous() and state.numel() >= _hip.URS_SLOTS):
        raise RuntimeError(f"lidarnerf.unet_train.{where}: the state must be a contiguous float64 tensor of {_hip.URS_SLOTS} slots")
    _hip.require_cuda(table, state)
    _hip.require_symbols(_STEP_SYMBOLS, "U-Net training")


def grad_sumsq(table, n_tensors, ws, state):
    """lnh_unet_grad_sumsq: state[URS_SUMSQ] = the float64 sum of grad^2 over the table's tensors, state[URS_NONFINITE] = 1 if any
    element is inf / NaN, else 0.  Fixed order, no float atomics."""
    _table_state(table, n_tensors, state, "grad_sumsq")
    _hip.require_cuda(ws)
    _hip.call("lnh_unet_grad_sumsq", _hip.ptr(table), int(n_tensors), _hip.ptr(ws), ws.numel() * ws.element_size(), _hip.ptr(state))
    return state


def rmsprop_step(table, n_tensors, state, loss_scale=1.0, max_norm=float("inf"), alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0):
    """lnh_unet_rmsprop_step: one launch for clip_grad_norm_(max_norm) on the gradients divided by loss_scale +
    torch.optim.RMSprop(foreach=True) over every tensor of the table, from grad_sumsq's state; the learning rate is
    state[URS_LR], read on the device.  A non-finite sum of squares skips the step: no tensor is written, state[URS_SKIPPED] += 1."""
    if float(momentum) > 0 and not getattr(table, "has_momentum_buffers", False):
        raise RuntimeError("lidarnerf.unet_train.rmsprop_step: momentum > 0 needs a table that step_table built with momentum_buffers "
                           "(this one has none, or is not step_table's: the kernel would follow a NULL pointer)")
    _table_state(table, n_tensors, state, "rmsprop_step")
    _hip.call("lnh_unet_rmsprop_step", _hip.ptr(table), int(n_tensors), _hip.ptr(state), float(loss_scale), float(max_norm), float(alpha),
              float(eps), float(weight_decay), float(momentum))
    return state
