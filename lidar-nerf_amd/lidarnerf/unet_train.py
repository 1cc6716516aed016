"""Training of the ray-drop U-Net of the mesh baselines (raydrop_train_poisson.py): what exists of it so far.
* The loss and the validation score of the reference's loop for the one-class net, as differentiable torch functions on any device
  and dtype; golden G18 pins them to the reference's own values.
* Backward kernels on tensors (csrc/unet_train.hip through the C ABI, include/lidarnerf_hip.h "U-Net training"): the max-pool
  backward with the skip add, the backward of the 1 x 1 head, the transposed convolution's weight pack, data gradient and weight / bias
  gradient.  One entry point each; they read no host memory and allocate nothing — the caller owns every buffer.  No CPU fallback.

The convolution and BatchNorm kernels of the training step, and with them the module that chains everything, are not in the package
yet: RayDropUNet keeps refusing training mode."""
import torch
import torch.nn.functional as F

from . import _hip
from .unet import _nhwc

_SYMBOLS = ("lnh_unet_pool_backward", "lnh_unet_head_backward", "lnh_unet_head_backward_workspace_size", "lnh_unet_pack_upconv",
            "lnh_unet_upconv2x2_backward_data", "lnh_unet_upconv2x2_backward_weight", "lnh_unet_upconv2x2_backward_weight_workspace_size")


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
    _hip.require_cuda(weight, dlogits, ws, dweight, dbias)
    need = head_backward_workspace_bytes(N, H, W)
    have = ws.numel() * ws.element_size()
    if have < need:
        raise RuntimeError(f"lidarnerf.unet_train.head_backward: the workspace holds {have} bytes, {need} needed")
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
    _hip.require_cuda(ws, dweight, dbias)
    need, have = upconv2x2_backward_weight_workspace_bytes(N, H, W, Cin, Cout), ws.numel() * ws.element_size()
    if have < need:
        raise RuntimeError(f"lidarnerf.unet_train.upconv2x2_backward_weight: the workspace holds {have} bytes, {need} needed")
    _hip.require_symbols(_SYMBOLS, "U-Net training")
    _hip.call("lnh_unet_upconv2x2_backward_weight", _hip.ptr(x), _hip.ptr(dy), Hd, Wd, Cs, int(offset), N, H, W, Cin, Cout, _hip.ptr(ws),
              have, _hip.ptr(dweight), _hip.ptr(dbias))
    return dweight, dbias
