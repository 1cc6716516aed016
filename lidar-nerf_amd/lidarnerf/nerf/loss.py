"""The LiDAR loss of the reference Trainer.train_step (lidarnerf/nerf/utils.py:712-876) under every loss option of its CLI:
the torch expressions (lidar_loss, patch_gradient_loss) and the one-launch kernels (fused_lidar_loss).  nerf/train_step.py
re-exports every name: LidarTrainer.loss is the dispatch between them."""
import ctypes as C
import dataclasses

import torch

from .. import _hip


_CRITERIA = ("l1", "mse", "huber", "bce")
_GRAD_CRITERIA = _CRITERIA + ("cos",)


@dataclasses.dataclass(frozen=True)
class LidarLossOptions:
    """The loss options of the reference CLI (main_lidarnerf.py:46-60, 92-103; criteria built at 330-342), under its names.
    The defaults are the loss the fast trainer has always trained: L1 depth, MSE ray-drop and intensity, and on patch
    epochs the non-Sobel L1 structural-gradient term.  alpha_d / alpha_r / alpha_i / alpha_grad and scale stay arguments of
    the callers (LidarTrainer's alpha_* and scale).  `huber` is HuberLoss(delta=0.2*scale), `bce` BCEWithLogitsLoss on
    the prediction as given, `cos` (depth_grad_loss only) 1 - CosineSimilarity per patch."""
    depth_loss: str = "l1"
    raydrop_loss: str = "mse"
    intensity_loss: str = "mse"
    depth_grad_loss: str = "l1"
    grad_loss: bool = True
    sobel_grad: bool = False
    grad_norm_smooth: bool = False
    spatial_smooth: bool = False
    tv_loss: bool = False
    alpha_grad_norm: float = 1.0
    alpha_spatial: float = 0.1
    alpha_tv: float = 1.0

    def __post_init__(self):
        for name in ("depth_loss", "raydrop_loss", "intensity_loss", "depth_grad_loss"):
            allowed = _GRAD_CRITERIA if name == "depth_grad_loss" else _CRITERIA
            v = getattr(self, name)
            if v not in allowed:
                raise ValueError(f"LidarLossOptions: {name}={v!r} is not one of {', '.join(allowed)}")
        for name in ("grad_loss", "sobel_grad", "grad_norm_smooth", "spatial_smooth", "tv_loss"):
            object.__setattr__(self, name, bool(getattr(self, name)))
        for name in ("alpha_grad_norm", "alpha_spatial", "alpha_tv"):
            object.__setattr__(self, name, float(getattr(self, name)))

    @classmethod
    def from_opt(cls, opt):
        """From a reference argparse namespace (main_lidarnerf.py); an attribute it lacks keeps this class's default."""
        return cls(**{f.name: getattr(opt, f.name, f.default) for f in dataclasses.fields(cls)})

    @property
    def is_default(self):
        return self == _DEFAULT_OPTIONS

    def huber_delta(self, scale):
        return 0.2 * float(scale)  # main_lidarnerf.py:336


_DEFAULT_OPTIONS = LidarLossOptions()


def _criterion(name, scale):
    """main_lidarnerf.py:330-342's loss_dict entry (reduction 'none')."""
    if name == "mse":
        return torch.nn.MSELoss(reduction="none")
    if name == "l1":
        return torch.nn.L1Loss(reduction="none")
    if name == "bce":
        return torch.nn.BCEWithLogitsLoss(reduction="none")
    if name == "huber":
        if scale is None:
            raise ValueError("the huber criterion needs the scene scale (delta = 0.2 * scale)")
        return torch.nn.HuberLoss(reduction="none", delta=0.2 * float(scale))
    return torch.nn.CosineSimilarity()


def lidar_loss(outputs, images_lidar, alpha_d=1000.0, alpha_r=1.0, alpha_i=10.0, *, options=None, scale=None):
    """utils.py:712-746; by default with the default criteria (L1 depth, MSE ray-drop, MSE intensity;
    main_lidarnerf.py:330-342), `options` (LidarLossOptions) selects others (`scale`: the huber delta's).
    images_lidar [B,N,3] = (raydrop, intensity, depth).  Returns (loss, pred_depth, gt_depth)."""
    gt_raydrop = images_lidar[..., 0]
    gt_intensity = images_lidar[..., 1] * gt_raydrop
    gt_depth = images_lidar[..., 2] * gt_raydrop
    pred_raydrop = outputs["image_lidar"][..., 0]
    pred_intensity = outputs["image_lidar"][..., 1] * gt_raydrop
    pred_depth = outputs["depth_lidar"] * gt_raydrop
    if options is None or options.is_default:
        per_ray = (alpha_d * (pred_depth - gt_depth).abs() + alpha_r * (pred_raydrop - gt_raydrop) ** 2
                   + alpha_i * (pred_intensity - gt_intensity) ** 2)
    else:
        per_ray = (alpha_d * _criterion(options.depth_loss, scale)(pred_depth, gt_depth)
                   + alpha_r * _criterion(options.raydrop_loss, scale)(pred_raydrop, gt_raydrop)
                   + alpha_i * _criterion(options.intensity_loss, scale)(pred_intensity, gt_intensity))
    return per_ray.mean(), pred_depth, gt_depth


class _FusedLidarLoss(torch.autograd.Function):
    """lidar_loss as ONE kernel that also emits d loss / d (depth, image); backward only scales by the upstream scalar."""

    @staticmethod
    def forward(ctx, depth, image, gt, ad, ar, ai, patch=None, grad_scale=None, options=None, scale=None, value_only=False):
        # patch = (px, py, scale, alpha_grad): the reference's patch epochs, structural-gradient term included
        # grad_scale (device scalar): the kernel multiplies the gradients it emits by it — the caller then starts
        # backward() from a gradient of ONE (LidarTrainer: the loss scale, without an element-wise launch in backward)
        # value_only: the render node has formed the gradients itself (fused.TRAIN_TAIL: default loss, no patch) — the same
        # kernel gives the value, with null gradient outputs, and backward hands nothing back
        n = depth.numel()
        depth, image, gt = depth.reshape(n).float().contiguous(), image.reshape(n, 2).float().contiguous(), \
            gt.reshape(n, 3).float().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=depth.device)
        ctx.value_only = bool(value_only)
        if value_only:
            if patch is not None or (options is not None and not options.is_default):
                raise ValueError("value_only: the default loss with one ray per patch only")
            _hip.call("lnh_lidar_loss", depth.data_ptr(), image.data_ptr(), gt.data_ptr(), n, float(ad), float(ar), float(ai),
                      None, loss.data_ptr(), None, None)
            return loss
        grads = torch.empty(3 * n, dtype=torch.float32, device=depth.device)  # [d/d depth (n) | d/d image (n, 2)]
        gs = None if grad_scale is None else grad_scale.data_ptr()
        if options is not None and not options.is_default:
            # lnh_lidar_loss_ex: every other option set (the default one keeps the two kernels below)
            _hip.require_version(102, "LidarLossOptions other than the defaults (lnh_lidar_loss_ex)")
            px, py, pscale, ag = patch if patch is not None else (1, 1, scale, 0.0)
            hscale = scale if scale is not None else pscale
            if hscale is None and "huber" in (options.depth_loss, options.raydrop_loss, options.intensity_loss,
                                              options.depth_grad_loss):
                raise ValueError("the huber criterion needs the scene scale (delta = 0.2 * scale)")
            opts = _hip.loss_options(options, px, py, 1.0 if pscale is None else pscale,
                                     0.0 if hscale is None else options.huber_delta(hscale), ad, ar, ai, ag)
            ws = torch.empty(int(_hip.lib().lnh_lidar_loss_ex_workspace_bytes(n)), dtype=torch.uint8, device=depth.device)
            _hip.call("lnh_lidar_loss_ex", depth.data_ptr(), image.data_ptr(), gt.data_ptr(), n, C.byref(opts), gs,
                      ws.data_ptr(), ws.numel(), loss.data_ptr(), grads.data_ptr(), grads.data_ptr() + 4 * n)
        elif patch is None:
            _hip.call("lnh_lidar_loss", depth.data_ptr(), image.data_ptr(), gt.data_ptr(), n, float(ad), float(ar), float(ai),
                      gs, loss.data_ptr(), grads.data_ptr(), grads.data_ptr() + 4 * n)
        else:
            px, py, scale, ag = patch
            _hip.call("lnh_lidar_loss_patch", depth.data_ptr(), image.data_ptr(), gt.data_ptr(), n, int(px), int(py),
                      float(scale), float(ad), float(ar), float(ai), float(ag), gs, loss.data_ptr(), grads.data_ptr(),
                      grads.data_ptr() + 4 * n)
        ctx.save_for_backward(grads)
        ctx.n, ctx.prescaled = n, grad_scale is not None
        return loss

    @staticmethod
    def backward(ctx, g):
        if ctx.value_only:
            return (None,) * 11
        (grads,) = ctx.saved_tensors
        # (pre-scaled gradients: the contract of grad_scale is that backward() starts from ONE)
        scaled = grads if ctx.prescaled else grads * g  # one launch for both
        return scaled[:ctx.n], scaled[ctx.n:].view(ctx.n, 2), None, None, None, None, None, None, None, None, None


class _ScaleGrad(torch.autograd.Function):
    """Identity whose gradient is multiplied by a device scalar (the loss scale, for the loss paths without a kernel)."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.save_for_backward(scale)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None


def fused_lidar_loss(outputs, images_lidar, alpha_d=1000.0, alpha_r=1.0, alpha_i=10.0, patch=None, grad_scale=None,
                     options=None, scale=None, value_only=False):
    """lidar_loss (+ patch_gradient_loss when patch = (px, py, scale, alpha_grad)) through the single-launch kernel (GPU
    tensors only); same value and gradients.  grad_scale (device scalar): the gradients come out multiplied by it and
    backward() must then be started from a gradient of one.  options (LidarLossOptions): any other loss option set of the
    reference CLI (lnh_lidar_loss_ex; `scale`, the huber delta's, defaults to the patch's).  value_only: `outputs` come
    from a render that took the training forward tail (outputs["train_tail"]) — the value alone, its gradients exist."""
    depth, image = outputs["depth_lidar"], outputs["image_lidar"]
    loss = _FusedLidarLoss.apply(depth.reshape(-1), image.reshape(-1, 2), images_lidar, alpha_d, alpha_r, alpha_i, patch,
                                 grad_scale, options, scale, value_only)
    return loss


_SOBEL_X = ((-1.0, 0.0, 1.0), (-2.0, 0.0, 2.0), (-1.0, 0.0, 1.0))
_SOBEL_Y = ((-1.0, -2.0, -1.0), (0.0, 0.0, 0.0), (1.0, 2.0, 1.0))


def patch_gradient_loss(pred_depth, gt_depth, gt_raydrop, px, py, scale, alpha_grad=100.0, *, options=None):
    """utils.py:760-876 (grad_loss, non-sobel): |dx| of the prediction vs the SIGNED dx of the ground truth, masked to
    |gt dx| < 0.01 m and returned rays; only the x term enters the loss (the y terms are computed but unused).
    `options` (LidarLossOptions): the reference's other patch terms — Sobel gradients, the smoothness terms, another
    depth_grad_loss criterion, grad_loss off — term for term as utils.py:760-876 writes them."""
    if options is None or options.is_default:
        pred = pred_depth.reshape(-1, 1, px, py) / scale
        gt = gt_depth.reshape(-1, 1, px, py) / scale
        rd = gt_raydrop.reshape(-1, 1, px, py)
        pred_gx = (pred[..., :-1] - pred[..., 1:]).abs()
        gt_gx = gt[..., :-1] - gt[..., 1:]
        mask = rd[..., :-1] * (gt_gx.abs() < 0.01)
        return alpha_grad * (pred_gx * mask - gt_gx * mask).abs().mean()
    o = options
    F = torch.nn.functional

    def sobel(x, k):
        return F.conv2d(x, torch.tensor(k, dtype=x.dtype, device=x.device)[None, None], padding=1)

    pred = pred_depth.reshape(-1, px, py, 1).permute(0, 3, 1, 2).contiguous() / scale
    if o.sobel_grad:
        pred_gx, pred_gy = sobel(pred, _SOBEL_X), sobel(pred, _SOBEL_Y)
    else:
        pred_gy = (pred[:, :, :-1, :] - pred[:, :, 1:, :]).abs()
        pred_gx = (pred[:, :, :, :-1] - pred[:, :, :, 1:]).abs()
    dy, dx = pred_gy.abs(), pred_gx.abs()
    loss = pred.new_zeros(())
    if o.grad_norm_smooth:
        loss = loss + o.alpha_grad_norm * (torch.exp(-dx).mean() + torch.exp(-dy).mean())
    if o.spatial_smooth:
        loss = loss + o.alpha_spatial * ((dx ** 2).mean() + (dy ** 2).mean())
    if o.tv_loss:
        loss = loss + o.alpha_tv * (dx.mean() + dy.mean())
    if o.grad_loss:
        gt = gt_depth.reshape(-1, px, py, 1).permute(0, 3, 1, 2).contiguous() / scale
        rd = gt_raydrop.reshape(-1, px, py, 1).permute(0, 3, 1, 2).contiguous()
        gt_gx = sobel(gt, _SOBEL_X) if o.sobel_grad else gt[:, :, :, :-1] - gt[:, :, :, 1:]
        mask = (rd if o.sobel_grad else rd[:, :, :, :-1]) * torch.where(gt_gx.abs() < 0.01, 1, 0)
        crit = _criterion(o.depth_grad_loss, scale)
        if o.depth_grad_loss == "cos":
            patches = pred_gx.shape[0]
            grad = 1 - crit((pred_gx * mask).reshape(patches, -1), (gt_gx * mask).reshape(patches, -1))
        else:
            grad = crit(pred_gx * mask, gt_gx * mask)
        loss = loss + alpha_grad * grad.mean()
    return loss
