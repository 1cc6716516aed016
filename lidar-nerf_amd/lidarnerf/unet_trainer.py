"""RayDropUNetTrainer: the training loop of raydrop_train_poisson.py:75-259 for a lidarnerf.unet.RayDropUNet on the device.
One step = unet_train.train_forward -> raydrop_unet_loss_and_grad -> train_backward(conv_weights=True) -> grad_sumsq -> rmsprop_step:
a linear chain of kernels on the current stream that reads no host memory, allocates nothing after the first call of a shape and can
be captured in a graph.  The reference's loop around it — evaluate(), ReduceLROnPlateau on the validation score, the checkpoint — is
restated on the host; the learning rate lives in device memory, so the scheduler changes it under a captured step.

Deviation from the reference's --amp loop, which clips the still-scaled gradients (it never calls unscale_): here the gradients are
divided by the (static) loss scale BEFORE clip_grad_norm_, as the float32 loop and golden G18's record do."""
import math
import os

import torch

from . import _hip
from . import unet as _unet
from . import unet_train as ut


def plateau_state(patience=5, factor=0.1, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8):
    """The state of torch.optim.lr_scheduler.ReduceLROnPlateau(mode="max", threshold_mode="rel"); the defaults are torch's but for
    the reference's patience of 5."""
    return {"best": -math.inf, "num_bad_epochs": 0, "cooldown_counter": 0, "last_epoch": 0, "factor": factor, "patience": patience,
            "threshold": threshold, "cooldown": cooldown, "min_lr": min_lr, "eps": eps}


def plateau_step(s, lr, score):
    """ReduceLROnPlateau.step(score) restated on the host: returns the learning rate after it.  A score counts as better if it is
    above best x (1 + threshold); after more than `patience` scores in a row that are not, lr <- max(factor lr, min_lr) where that
    lowers it by more than eps."""
    s["last_epoch"] += 1
    if score > s["best"] * (s["threshold"] + 1.0):
        s["best"], s["num_bad_epochs"] = score, 0
    else:
        s["num_bad_epochs"] += 1
    if s["cooldown_counter"] > 0:
        s["cooldown_counter"] -= 1
        s["num_bad_epochs"] = 0
    if s["num_bad_epochs"] > s["patience"]:
        new_lr = max(lr * s["factor"], s["min_lr"])
        if lr - new_lr > s["eps"]:
            lr = new_lr
        s["cooldown_counter"], s["num_bad_epochs"] = s["cooldown"], 0
    return lr


def rmsprop_state_dict(step, square_avgs, momentum_buffers, lr, alpha, eps, weight_decay, momentum):
    """A state_dict in torch.optim.RMSprop's own layout: per parameter `step` (a float32 scalar on the CPU, as torch keeps it),
    `square_avg` and, with momentum > 0, `momentum_buffer`; one param group with torch's keys.  No state before the first step, as
    in torch."""
    proto = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(1))], lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay,
                                momentum=momentum, foreach=True)
    group = dict(proto.state_dict()["param_groups"][0], params=list(range(len(square_avgs))))
    state = {}
    if step > 0:
        for i, sq in enumerate(square_avgs):
            state[i] = {"step": torch.tensor(float(step)), "square_avg": sq}
            if momentum > 0:
                state[i]["momentum_buffer"] = momentum_buffers[i]
    return {"state": state, "param_groups": [group]}


class RayDropUNetTrainer:
    """RMSprop + gradient clipping + static loss scale around a RayDropUNet; the defaults are train_model's.  The net stays in
    whatever mode it is in (RayDropUNet itself refuses training mode); its parameters are updated in place and must not be moved
    or replaced while the trainer lives."""

    def __init__(self, net, lr=1e-5, weight_decay=1e-8, momentum=0.999, alpha=0.99, eps=1e-8, gradient_clipping=1.0, loss_scale=1024.0,
                 graph=False):
        if not isinstance(net, _unet.RayDropUNet):
            raise TypeError("RayDropUNetTrainer: net must be a lidarnerf.unet.RayDropUNet")
        self._named = list(net.named_parameters())
        if not self._named or not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for _, p in self._named):
            raise RuntimeError("RayDropUNetTrainer: the net's parameters must be contiguous f32 tensors on the GPU (no CPU fallback)")
        if not (lr >= 0 and weight_decay >= 0 and momentum >= 0 and alpha >= 0 and eps >= 0 and gradient_clipping > 0 and
                0 < loss_scale < math.inf):
            raise ValueError("RayDropUNetTrainer: lr, weight_decay, momentum, alpha, eps must be >= 0; gradient_clipping and a finite "
                             "loss_scale > 0")
        _hip.require_symbols(_unet._SYMBOLS + ut._SYMBOLS + ut._STEP_SYMBOLS, "U-Net training")
        self.net, self.graph = net, bool(graph)
        self.lr, self.weight_decay, self.momentum, self.alpha, self.eps = float(lr), float(weight_decay), float(momentum), float(alpha), float(eps)
        self.gradient_clipping, self.loss_scale = float(gradient_clipping), float(loss_scale)
        self.device = self._named[0][1].device
        self._ptrs = [p.data_ptr() for _, p in self._named]
        # square_avg and momentum_buffer: one flat allocation each, every tensor's view starting on 16 bytes
        offs, total = [], 0
        for _, p in self._named:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        self._sq_flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._buf_flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.square_avg = [self._sq_flat[o:o + p.numel()].view(p.shape) for o, (_, p) in zip(offs, self._named)]
        self.momentum_buffer = [self._buf_flat[o:o + p.numel()].view(p.shape) for o, (_, p) in zip(offs, self._named)]
        self.state = torch.zeros(_hip.URS_SLOTS, dtype=torch.float64, device=self.device)  # LNH_URS_* slots
        self.state[_hip.URS_LR] = self.lr
        self._ws_sumsq = torch.empty(ut.grad_sumsq_workspace_bytes(), dtype=torch.uint8, device=self.device)
        self._epoch_loss = torch.zeros((), dtype=torch.float32, device=self.device)
        self._ctx = {}
        # ReduceLROnPlateau(mode="max", patience=5), torch's defaults
        self.scheduler = plateau_state()

    # -- one step --
    def _context(self, st, images, masks):
        N, H, W = st["key"][:3]
        grads = [st["grads"][name] for name, _ in self._named]
        M = N * H * W
        u8 = masks.dtype in (torch.uint8, torch.bool)
        ctx = {"state": st, "images": torch.empty(images.shape, dtype=torch.float32, device=self.device) if self.graph else None,
               "masks": torch.empty(M, dtype=torch.uint8 if u8 else torch.float32, device=self.device),
               "dlogits": torch.empty(N, 1, H, W, dtype=torch.float32, device=self.device),
               "loss": torch.zeros(1, dtype=torch.float32, device=self.device),
               "ws_loss": torch.empty(ut.loss_grad_workspace_bytes(M), dtype=torch.uint8, device=self.device),
               "table": ut.step_table([p.detach() for _, p in self._named], grads, self.square_avg, self.momentum_buffer),
               "graph": None, "calls": 0}
        ctx["loss_out"] = ctx["loss"].view(())
        return ctx

    def _chain(self, ctx, images):
        """The device work of one step on ctx's buffers.  (train_forward hands back the cached state of the shape: ctx's.)"""
        n = len(self._named)
        logits, st = ut.train_forward(self.net, images, ctx["state"])
        ut.raydrop_unet_loss_and_grad(logits, ctx["masks"], ctx["dlogits"], ctx["loss"], ctx["ws_loss"], self.loss_scale)
        ut.train_backward(self.net, st, ctx["dlogits"], conv_weights=True)
        ut.grad_sumsq(ctx["table"], n, self._ws_sumsq, self.state)
        ut.rmsprop_step(ctx["table"], n, self.state, self.loss_scale, self.gradient_clipping, self.alpha, self.eps, self.weight_decay,
                        self.momentum)

    def train_step(self, images, masks):
        """One step of the reference's loop on a batch: images f32 [N, n_channels, H, W], masks [N, H, W] (or [N, 1, H, W]) of 0 / 1 in
        any dtype, both on the GPU -> the loss of the batch BEFORE the update, a 0-dim f32 device tensor that the next step of the
        shape overwrites.  No host read; after the first call of a shape no allocation and no synchronisation.  With graph=True the
        step of a shape is captured at its second call (the first runs eagerly and makes the buffers) and replayed from then on."""
        if not (torch.is_tensor(images) and images.dim() == 4 and images.is_cuda and torch.is_tensor(masks) and masks.is_cuda):
            raise RuntimeError("RayDropUNetTrainer.train_step: images [N, C, H, W] and masks must be GPU tensors (no CPU fallback)")
        N, _, H, W = images.shape
        if masks.numel() != N * H * W:
            raise ValueError(f"RayDropUNetTrainer.train_step: masks of {tuple(masks.shape)} do not fit images of {tuple(images.shape)}")
        if [p.data_ptr() for _, p in self._named] != self._ptrs:
            raise RuntimeError("RayDropUNetTrainer: the net's parameters were moved or replaced; make a new trainer")
        key = (N, H, W)
        ctx = self._ctx.get(key)
        if ctx is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RayDropUNetTrainer: the first step of a shape cannot be captured (run it eagerly once)")
            st = ut._train_state(self.net, N, H, W, images.device)
            ctx = self._ctx[key] = self._context(st, images, masks)
        ctx["masks"].view(masks.shape).copy_(masks)
        ctx["calls"] += 1
        if not self.graph:
            self._chain(ctx, images)
            return ctx["loss_out"]
        ctx["images"].copy_(images)
        if ctx["graph"] is None and ctx["calls"] >= 2:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._chain(ctx, ctx["images"])
            ctx["graph"] = g
        if ctx["graph"] is None:
            self._chain(ctx, ctx["images"])
        else:
            ctx["graph"].replay()
            # what train_forward's last Python line does in an eager step and a replay does not run: the parameters and running
            # statistics have changed, so the net's cached inference pack is stale (the next inference call packs again)
            self.net._packed = None
        return ctx["loss_out"]

    def train_epoch(self, batches):
        """train_step over an iterable of (images, masks); the mean loss as a float — the one host read of the epoch."""
        self._epoch_loss.zero_()
        n = 0
        for images, masks in batches:
            self._epoch_loss.add_(self.train_step(images, masks))
            n += 1
        return float(self._epoch_loss) / max(n, 1)

    # -- the loop around it --
    @torch.no_grad()
    def evaluate(self, batches):
        """The reference's evaluate(): the inference forward (running statistics) and raydrop_unet_dice_score per batch, averaged
        over the batches (divided by max(number of batches, 1)); a 0-dim device tensor."""
        was_training = self.net.training
        self.net.eval()
        try:
            score, n = torch.zeros((), dtype=torch.float32, device=self.device), 0
            for images, masks in batches:
                score += ut.raydrop_unet_dice_score(self.net(images), masks.to(self.device))
                n += 1
        finally:
            self.net.train(was_training)
        return score / max(n, 1)

    def set_lr(self, lr):
        self.lr = float(lr)
        self.state[_hip.URS_LR:_hip.URS_LR + 1].fill_(self.lr)

    def scheduler_step(self, score):
        """plateau_step on the trainer's scheduler state (a host read if `score` is a device tensor); writes the device's lr."""
        new_lr = plateau_step(self.scheduler, self.lr, float(score))
        if new_lr != self.lr:
            self.set_lr(new_lr)
        return self.lr

    # -- state --
    def _counters(self):
        host = self.state.cpu()
        return int(host[_hip.URS_STEP]), int(host[_hip.URS_SKIPPED])

    @property
    def steps(self):
        """(steps taken, steps skipped for a non-finite gradient): a host read."""
        return self._counters()

    def optimizer_state_dict(self):
        """torch.optim.RMSprop's own state_dict layout — per parameter `step`, `square_avg`, `momentum_buffer`, one param group — so
        a stock RMSprop over the stock UNet's parameters loads it; tensors are copies on the trainer's device."""
        return rmsprop_state_dict(self._counters()[0], [t.clone() for t in self.square_avg], [t.clone() for t in self.momentum_buffer],
                                  lr=self.lr, alpha=self.alpha, eps=self.eps, weight_decay=self.weight_decay, momentum=self.momentum)

    def load_optimizer_state_dict(self, sd):
        """The inverse: a state_dict of torch.optim.RMSprop (or optimizer_state_dict's) over the same 64 parameters in order.  Takes
        lr, alpha, eps, weight_decay and momentum of its group, the step count and every state tensor.  Steps already captured are
        dropped (they hold the old hyperparameters as kernel arguments); the next call of a shape captures again."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._named):
            raise ValueError(f"RayDropUNetTrainer: expected one param group of {len(self._named)} parameters")
        g = groups[0]
        if g.get("centered"):
            raise NotImplementedError("RayDropUNetTrainer: centered RMSprop")
        state = sd["state"]
        if state and sorted(state) != sorted(g["params"]):
            raise ValueError("RayDropUNetTrainer: the state must cover every parameter or none")
        self.alpha, self.eps, self.weight_decay, self.momentum = float(g["alpha"]), float(g["eps"]), float(g["weight_decay"]), float(g["momentum"])
        for ctx in self._ctx.values():  # these are kernel arguments of a captured step (only lr lives on the device): capture again
            ctx["graph"] = None
        self._sq_flat.zero_()
        self._buf_flat.zero_()
        step = 0
        for i, pid in enumerate(g["params"]):
            if not state:
                break
            s = state[pid]
            if tuple(s["square_avg"].shape) != tuple(self._named[i][1].shape):
                raise ValueError(f"RayDropUNetTrainer: square_avg of parameter {i} has shape {tuple(s['square_avg'].shape)}")
            self.square_avg[i].copy_(s["square_avg"])
            if "momentum_buffer" in s and s["momentum_buffer"] is not None:
                self.momentum_buffer[i].copy_(s["momentum_buffer"])
            step = int(float(s["step"]))
        self.state[_hip.URS_STEP:_hip.URS_STEP + 1].fill_(float(step))
        self.set_lr(g["lr"])

    @staticmethod
    def optimizer_path(path):
        return str(path) + ".optim"

    def save_checkpoint(self, path):
        """`path`: the net's state_dict(), as the reference writes it (RayDropUNet.from_checkpoint and the reference's UNet load it);
        `path`.optim beside it: the optimizer state, the scheduler's and the skipped-step count."""
        torch.save({k: v.detach().cpu() for k, v in self.net.state_dict().items()}, path)
        opt = self.optimizer_state_dict()
        opt["state"] = {i: {k: v.cpu() for k, v in s.items()} for i, s in opt["state"].items()}
        torch.save({"optimizer": opt, "scheduler": dict(self.scheduler), "skipped": self._counters()[1]}, self.optimizer_path(path))

    def load_checkpoint(self, path):
        """Load `path` into the net in place and, if it is there, `path`.optim into the trainer."""
        self.net.load_state_dict(torch.load(path, map_location="cpu"))
        if os.path.exists(self.optimizer_path(path)):
            extra = torch.load(self.optimizer_path(path), map_location="cpu")
            self.load_optimizer_state_dict(extra["optimizer"])
            self.scheduler.update(extra["scheduler"])
            self.state[_hip.URS_SKIPPED:_hip.URS_SKIPPED + 1].fill_(float(extra["skipped"]))
