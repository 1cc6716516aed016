"""The ray-drop MLP of the PCGen baseline and its training loop on the device (lidarnvs/raydrop_train_pcgen.py: RayDrop,
run_network, train) — csrc/raydrop.hip, contract in include/lidarnerf_hip.h (lnh_raydrop_*) and DESIGN §17.

RayDropMLP is the reference's `RayDrop` behind `run_network` with the identity embedding (i_embed = -1, the reference's default
and what its consumer lidarnvs_pcgen.py hard-wires): rows (direction x, y, z, depth, intensity) -> D x (Linear(W) + ReLU) ->
Linear(1), fp32 throughout.  RayDropTrainer is the loop of train(): contiguous batches of a shuffled table, img2mse / mseloss /
l1loss, torch.optim.Adam, the exponential or the warm-up + cosine learning-rate schedule with the reference's one-step lag.  A
step is three launches (forward + backward rows, weight gradients, Adam) and no host read.

Not reproduced (the precedent of DESIGN §6.4): the initial np.random.shuffle of the table and torch.randperm's CPU stream — the
trainer shuffles on the device from its own seed.  The positional-encoding option (i_embed = 0) is refused.  No CPU fallback."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _hip

IN_FEATURES = 5
LOSS_TYPES = {"img2mse": 0, "mseloss": 0, "l1loss": 1}
_SYMBOLS = ("lnh_raydrop_forward", "lnh_raydrop_grad", "lnh_raydrop_adam", "lnh_raydrop_workspace_size",
            "lnh_raydrop_param_count")


def param_count(D, W):
    return W * IN_FEATURES + W + (D - 1) * (W * W + W) + W + 1


def _check_shape(D, W):
    if W not in (128, 256) or not 1 <= D <= 8:
        raise ValueError(f"RayDropMLP: W must be 128 or 256 and 1 <= D <= 8 (got D={D}, W={W})")


class _Linear(nn.Module):
    """weight / bias of one nn.Linear as views of the flat buffer (the names of the reference's state dict)."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight, self.bias = nn.Parameter(weight, requires_grad=False), nn.Parameter(bias, requires_grad=False)


class RayDropMLP(nn.Module):
    """D hidden layers of width W (the consumer's 4 x 128; the training CLI's default is 8 x 256).  Every parameter is a view of
    ONE flat fp32 buffer `flat` in torch's own layout (linears.0.weight, linears.0.bias, ..., output_linear.weight,
    output_linear.bias), so load_state_dict takes the reference's ckpt["network_fn_state_dict"] unchanged and the kernels read
    the buffer as it is.  Initialisation is the reference's weights_init: kaiming-normal weights, zero biases."""

    def __init__(self, D=4, W=128, i_embed=-1):
        super().__init__()
        D, W = int(D), int(W)
        _check_shape(D, W)
        if i_embed != -1:
            raise NotImplementedError("RayDropMLP: only the identity embedding (i_embed = -1) is built; the positional "
                                      "encoding of the reference's i_embed = 0 is out of scope")
        self.D, self.W = D, W
        self.num_parameters = param_count(D, W)
        self._bind(torch.zeros(self.num_parameters, dtype=torch.float32))
        for lin in list(self.linears) + [self.output_linear]:
            nn.init.kaiming_normal_(lin.weight.data)
            nn.init.zeros_(lin.bias.data)

    def _bind(self, flat):
        """(Re)build the views on a flat buffer."""
        self.flat = flat
        views, o = [], 0
        for l in range(self.D + 1):
            rows, cols = (self.W, IN_FEATURES if l == 0 else self.W) if l < self.D else (1, self.W)
            w = flat[o:o + rows * cols].view(rows, cols)
            o += rows * cols
            views.append(_Linear(w, flat[o:o + rows]))
            o += rows
        assert o == self.num_parameters
        self.linears = nn.ModuleList(views[:-1])
        self.output_linear = views[-1]

    def _apply(self, fn, recurse=True):  # .cuda() / .to(): move the flat buffer once and rebuild the views on it
        flat = fn(self.flat)
        if flat.dtype != torch.float32:
            raise TypeError("RayDropMLP is fp32 only")
        self._bind(flat.contiguous())
        return self

    def _rows(self, rows, who):
        if not torch.is_tensor(rows) or not rows.is_cuda or not self.flat.is_cuda:
            raise RuntimeError(f"RayDropMLP.{who}: the model and its rows must live on the GPU (no CPU fallback)")
        if rows.dim() != 2 or rows.shape[1] < IN_FEATURES or rows.dtype != torch.float32:
            raise ValueError(f"RayDropMLP.{who}: rows must be float32 [N, >= 5] (direction, depth, intensity), got "
                             f"{rows.dtype} {tuple(rows.shape)}")
        if rows.device != self.flat.device:
            raise RuntimeError(f"RayDropMLP.{who}: rows on {rows.device}, the model on {self.flat.device}")
        return rows.detach().contiguous()

    @torch.no_grad()
    def forward(self, rows):
        """rows f32 [N, >= 5] on the GPU -> the raw network output [N, 1] (no sigmoid, as in the reference).  Inference only:
        training goes through RayDropTrainer."""
        _hip.require_symbols(_SYMBOLS, "the ray-drop MLP")
        rows = self._rows(rows, "forward")
        out = torch.empty((rows.shape[0], 1), dtype=torch.float32, device=rows.device)
        with torch.cuda.device(rows.device):
            _hip.call("lnh_raydrop_forward", self.flat.data_ptr(), self.D, self.W, rows.data_ptr(), rows.shape[1], rows.shape[0],
                      out.data_ptr())
        return out

    def predict_mask(self, rows):
        """1.0 where the ray is kept (output > 0.5), else 0.0: [N, 1]."""
        return (self.forward(rows) > 0.5).to(torch.float32)


def cosine_schedule(base_value, final_value, steps, warmup_iters=0, start_warmup_value=0.0):
    """cosine_scheduler of raydrop_train_pcgen.py:205-219 in float64."""
    steps, warmup_iters = int(steps), int(warmup_iters)
    if steps <= warmup_iters:
        raise ValueError(f"cosine schedule: {steps} steps do not outlast the warm-up of {warmup_iters}")
    warm = np.linspace(start_warmup_value, base_value, warmup_iters) if warmup_iters > 0 else np.array([])
    iters = np.arange(steps - warmup_iters)
    sched = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * iters / len(iters)))
    return np.concatenate((warm, sched))


def lr_table(N_iters, lrate=5e-4, lrate_decay=500, cosLR=False, coslrate=5e-4, cosminlrate=5e-5, warmup_iters=1000):
    """float64 [N_iters]: the learning rate step k = 0, 1, ... of the reference's loop runs at.  The reference sets the rate
    AFTER optimizer.step() from the count of completed steps minus one (raydrop_train_pcgen.py:475-482), so the first step runs
    at `lrate` whichever schedule is chosen and step k >= 1 at the schedule's entry k - 1."""
    N_iters = int(N_iters)
    if N_iters < 1:
        raise ValueError("lr_table: N_iters must be at least 1")
    if cosLR:
        sched = cosine_schedule(coslrate, cosminlrate, N_iters, warmup_iters)
    else:
        sched = lrate * (0.1 ** (np.arange(N_iters, dtype=np.float64) / (lrate_decay * 1000)))
    return np.concatenate(([float(lrate)], sched[:N_iters - 1]))


class RayDropTrainer:
    """The loop of raydrop_train_pcgen.py:train() on the device.  rows: the [M, 6] f32 table (direction, depth, intensity,
    target) on the model's GPU, in the order the first epoch walks it (the reference shuffles it once on the host before the
    loop: do that, or not, before handing it over).  step() runs the batch rows[i : i + N_rand] — the last batch of an epoch is
    short, as the reference's slice is — and when i >= M reshuffles the table with torch.randperm on the device (generator
    seeded with `seed`) and starts over.  No step reads the host."""

    def __init__(self, model, rows, N_rand=2048, lrate=5e-4, lrate_decay=500, cosLR=False, coslrate=5e-4, cosminlrate=5e-5,
                 warmup_iters=1000, N_iters=500000, loss="img2mse", seed=0):
        _hip.require_symbols(_SYMBOLS, "the ray-drop trainer")
        if not isinstance(model, RayDropMLP) or not model.flat.is_cuda:
            raise RuntimeError("RayDropTrainer: model must be a RayDropMLP on the GPU (no CPU fallback)")
        if loss not in LOSS_TYPES:
            raise ValueError(f"RayDropTrainer: loss must be one of {sorted(LOSS_TYPES)}, got {loss!r}")
        if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] != 6 or rows.dtype != torch.float32 or rows.shape[0] < 1:
            raise ValueError("RayDropTrainer: rows must be a float32 [M, 6] tensor with M >= 1")
        if rows.device != model.flat.device:
            raise RuntimeError(f"RayDropTrainer: rows on {rows.device}, the model on {model.flat.device}")
        if int(N_rand) < 1:
            raise ValueError("RayDropTrainer: N_rand must be at least 1")
        self.model, self.device = model, model.flat.device
        self.rows = rows.detach().contiguous()
        self.N_rand, self.loss_name, self.loss_type = int(N_rand), loss, LOSS_TYPES[loss]
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.lr_schedule = lr_table(N_iters, lrate, lrate_decay, cosLR, coslrate, cosminlrate, warmup_iters)
        self.lr_table = torch.from_numpy(self.lr_schedule.astype(np.float32)).to(self.device)
        P = model.num_parameters
        self.exp_avg = torch.zeros(P, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.grad = torch.zeros_like(self.exp_avg)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._steps = torch.zeros(2, dtype=torch.float32, device=self.device)  # the Adam step count, double-buffered
        self._cur = 0
        B = min(self.N_rand, self.rows.shape[0])
        self._ws = torch.empty(int(_hip.lib().lnh_raydrop_workspace_size(model.D, model.W, B)), dtype=torch.uint8,
                               device=self.device)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self.cursor = 0
        self.global_step = 0  # completed steps

    @property
    def adam_step(self):
        """The device-side Adam step count (one host read)."""
        return int(self._steps[self._cur].item())

    def grad_step(self, batch):
        """loss and gradients of one [B, 6] batch into self.loss / self.grad (overwritten); B <= min(N_rand, M)."""
        m = self.model
        _hip.call("lnh_raydrop_grad", m.flat.data_ptr(), m.D, m.W, batch.data_ptr(), batch.shape[0], self.loss_type,
                  self._ws.data_ptr(), self._ws.numel(), self.loss.data_ptr(), self.grad.data_ptr())

    def adam_step_(self):
        s = self._steps
        _hip.call("lnh_raydrop_adam", self.model.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                  self.grad.data_ptr(), self.model.num_parameters, self.lr_table.data_ptr(), self.lr_table.numel(),
                  s.data_ptr() + 4 * self._cur, s.data_ptr() + 4 * (1 - self._cur), *self.betas, self.eps)
        self._cur = 1 - self._cur

    def step(self):
        """One optimisation step; returns the [1] device tensor the loss of this step is written to (no host read)."""
        M = self.rows.shape[0]
        with torch.cuda.device(self.device):
            batch = self.rows[self.cursor:self.cursor + self.N_rand]
            self.grad_step(batch)
            self.adam_step_()
            self.cursor += self.N_rand
            if self.cursor >= M:
                self.rows = self.rows[torch.randperm(M, device=self.device, generator=self.generator)]
                self.cursor = 0
        self.global_step += 1
        return self.loss

    def train(self, n):
        """n steps; the loss of the last one as a Python float (the only host read)."""
        for _ in range(int(n)):
            self.step()
        return float(self.loss.item())

    # ------------------------------------------------------------------------------------------------------ checkpoints
    def optimizer_state_dict(self):
        """torch.optim.Adam's state-dict layout over the model's parameters in order, so a stock torch.optim.Adam over
        modules of the same names loads it."""
        params = list(self.model.parameters())
        lr = float(self.lr_schedule[min(self.global_step, len(self.lr_schedule) - 1)])
        host = [nn.Parameter(torch.zeros(1)) for _ in params]
        group = torch.optim.Adam(host, lr=lr, betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        group["params"] = list(range(len(params)))
        state, o = {}, 0
        step = float(self._steps[self._cur].item())
        if step > 0:
            for k, p in enumerate(params):
                n = p.numel()
                state[k] = {"step": torch.tensor(step, dtype=torch.float32),
                            "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
                o += n
        return {"state": state, "param_groups": [group]}

    def save_checkpoint(self, path):
        """The reference's keys (global_step, network_fn_state_dict, optimizer_state_dict) plus `sampler_state`: the batch cursor
        and the shuffle generator's state.  The table itself is not stored: a run continues bit-identically on a trainer whose
        table is in the order this one's is in."""
        torch.save({"global_step": self.global_step,
                    "network_fn_state_dict": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
                    "optimizer_state_dict": self.optimizer_state_dict(),
                    "sampler_state": {"cursor": self.cursor, "generator": self.generator.get_state()}}, path)

    def load_checkpoint(self, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ckpt["network_fn_state_dict"])
        state = ckpt["optimizer_state_dict"]["state"]
        params = list(self.model.parameters())
        self.exp_avg.zero_(), self.exp_avg_sq.zero_()
        step, o = 0.0, 0
        for k, p in enumerate(params):
            n = p.numel()
            if k in state:
                self.exp_avg[o:o + n].copy_(state[k]["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(state[k]["exp_avg_sq"].reshape(-1))
                step = float(state[k]["step"])
            o += n
        self._steps[self._cur] = step
        self.global_step = int(ckpt["global_step"])
        sampler = ckpt.get("sampler_state")
        if sampler is not None:
            self.cursor = int(sampler["cursor"])
            self.generator.set_state(sampler["generator"])
        return ckpt
