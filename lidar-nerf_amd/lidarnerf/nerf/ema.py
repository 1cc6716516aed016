"""Exponential moving average of the parameters, with the interface of torch_ema.ExponentialMovingAverage — the class the
reference trainer builds (nerf/utils.py:619-624, decay 0.95 from main_lidarnerf.py:431), updates once per epoch
(1257-1258), swaps in for every evaluation (1297-1299, 1444-1445) and carries in its checkpoints under "ema"
(1463-1464, 1538-1539).

This module RESTATES torch_ema from its published formula; no build of that package was available to pin it against
(unpinned vs a real torch_ema build):

    update():  num_updates += 1;  decay = min(decay, (1 + num_updates) / (10 + num_updates))   (use_num_updates)
               one_minus_decay = 1.0 - decay                                                    (Python double)
               tmp = shadow - param;  tmp.mul_(one_minus_decay);  shadow.sub_(tmp)              (per parameter)
    state_dict(): {"decay", "num_updates", "shadow_params", "collected_params"}

On the GPU the parameter pass is HIP (csrc/ema.hip): ONE lnh_ema_update launch for the hash table and the small fp32
tensors, bit-identical to the three torch operations above, and swap() — one lnh_ema_swap launch that exchanges
parameters and shadows in place and rewrites the persistent fp16 compute copy of the table (`_lnh_table16`, kept by
LidarTrainer's fused table optimizer) in the same pass.  swap() twice is what store() + copy_to() ... restore() do, without
a third copy of the parameters.  Both kernels write through raw pointers: no torch version counter moves, no pointer
changes, a captured training step stays valid.

Tensors the launch does not take (more than LNH_TRAIN_MAX_SMALL small ones, non-fp32 or non-contiguous ones) and every
tensor on the CPU go through the same formula as torch operations: this is host-side trainer state, like the optimizer's
state dict — not a CPU path of a render kernel.
"""
import contextlib

import torch


class ParameterEMA:
    def __init__(self, parameters, decay, use_num_updates=True):
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self._params = list(parameters)
        # fp32 clones in the order given, every parameter whether or not it requires a gradient
        self.shadow_params = [p.detach().clone().float() if p.is_floating_point() else p.detach().clone()
                              for p in self._params]
        self.collected_params = None
        self.last_decay = None  # the decay the last update() applied (after the warm-up rule)

    # ------------------------------------------------------------------------------------------------ helpers
    def _get_parameters(self, parameters):
        if parameters is None:
            return self._params
        parameters = list(parameters)
        if len(parameters) != len(self.shadow_params):
            raise ValueError(f"Number of parameters passed as argument ({len(parameters)}) is different from the number of "
                             f"shadow parameters maintained by this ParameterEMA ({len(self.shadow_params)})")
        return parameters

    @staticmethod
    def _check_whole(params):
        for p in params:
            if getattr(p, "_lnh_master_stale", False):
                raise RuntimeError("ParameterEMA: the fp32 hash table is current on this rank's rows only (sharded table "
                                   "optimizer): call LidarTrainer.gather_table_state() on every rank first — "
                                   "LidarTrainer.ema_update() / ema_weights() do")

    def _plan(self, params):
        """Which tensors one launch takes: (table index or None, [small indices], [indices left to torch ops])."""
        idx = range(len(params))
        if not params or not all(p.is_cuda for p in params) or len({p.device for p in params}) != 1:
            return None, [], list(idx)
        ok = [i for i in idx if params[i].dtype == torch.float32 and params[i].is_contiguous()
              and self.shadow_params[i].dtype == torch.float32 and self.shadow_params[i].is_contiguous()
              and self.shadow_params[i].device == params[i].device and 0 < params[i].numel() < 2 ** 32]
        aligned = [i for i in ok if (params[i].data_ptr() | self.shadow_params[i].data_ptr()) % 16 == 0]
        table = next((i for i in aligned if getattr(params[i], "_lnh_table16", None) is not None), None)
        if table is None and aligned:
            table = max(aligned, key=lambda i: params[i].numel())
        from .. import _hip
        small = [i for i in ok if i != table][:_hip.TRAIN_MAX_SMALL]
        taken = set(small) | ({table} if table is not None else set())
        return table, small, [i for i in idx if i not in taken]

    def _launch(self, name, params, table, small, tail_args):
        from .. import _hip
        H = _hip
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"ParameterEMA: {name} must not be issued while a stream is capturing (run it between steps)")
        sh = self.shadow_params
        cast = lambda arr: H.C.cast(arr, H.C.c_void_p)
        pp = H.ptr_array([params[i].data_ptr() for i in small])
        ss = H.ptr_array([sh[i].data_ptr() for i in small])
        nn_ = H.u32_array([params[i].numel() for i in small])
        tp = params[table] if table is not None else None
        n = tp.numel() if tp is not None else 0
        if name == "lnh_ema_update":
            _hip.call(name, sh[table].data_ptr() if tp is not None else None, tp.data_ptr() if tp is not None else None, n,
                      cast(ss), cast(pp), cast(nn_), len(small), *tail_args)
        else:
            _hip.call(name, tp.data_ptr() if tp is not None else None, sh[table].data_ptr() if tp is not None else None,
                      tail_args[0], n, cast(pp), cast(ss), cast(nn_), len(small))

    @staticmethod
    def _table16(p):
        """The persistent fp16 compute copy of a parameter (fused table optimizer), or None."""
        t16 = getattr(p, "_lnh_table16", None)
        if t16 is not None and not (t16.dtype == torch.float16 and t16.numel() == p.numel() and t16.device == p.device
                                    and t16.is_contiguous()):
            raise RuntimeError("ParameterEMA: the fp16 compute copy of the table does not match its parameter")
        return t16

    def _refresh16(self, params):
        for p in params:
            t16 = self._table16(p)
            if t16 is not None:
                t16.copy_(p.detach().reshape(t16.shape))

    # ------------------------------------------------------------------------------------------------ torch_ema's interface
    def update(self, parameters=None):
        """One averaging step over all parameters (the reference calls it once per epoch)."""
        params = self._get_parameters(parameters)
        self._check_whole(params)
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = min(decay, (1 + self.num_updates) / (10 + self.num_updates))
        self.last_decay = decay
        one_minus_decay = 1.0 - decay
        with torch.no_grad():
            table, small, rest = self._plan(params)
            if table is not None or small:
                self._launch("lnh_ema_update", params, table, small, (one_minus_decay,))
            for i in rest:
                s, p = self.shadow_params[i], params[i]
                if not s.is_floating_point():
                    s.copy_(p)
                    continue
                tmp = s - p.detach().to(s.device)
                tmp.mul_(one_minus_decay)
                s.sub_(tmp)

    def swap(self, parameters=None):
        """Exchange parameters and shadows in place (and rewrite the fp16 compute copy of the table from its new
        contents).  swap() ... swap() is store() + copy_to() ... restore() without a third copy of the parameters."""
        params = self._get_parameters(parameters)
        self._check_whole(params)
        with torch.no_grad():
            table, small, rest = self._plan(params)
            if table is not None or small:
                t16 = self._table16(params[table]) if table is not None else None
                self._launch("lnh_ema_swap", params, table, small, (t16.data_ptr() if t16 is not None else None,))
            for i in rest:
                s, p = self.shadow_params[i], params[i]
                tmp = p.detach().clone()
                p.data.copy_(s)
                s.copy_(tmp)
            # (the launch has written the fp16 copy of ITS table; any other parameter that keeps one is re-cast)
            self._refresh16([params[i] for i in rest] + [params[i] for i in small])

    def store(self, parameters=None):
        """Keep a copy of the current parameters for restore()."""
        params = self._get_parameters(parameters)
        self._check_whole(params)
        self.collected_params = [p.detach().clone() for p in params]

    def copy_to(self, parameters=None):
        """Write the averaged values into the parameters (through `.data`, as torch_ema does)."""
        params = self._get_parameters(parameters)
        self._check_whole(params)
        with torch.no_grad():
            for s, p in zip(self.shadow_params, params):
                p.data.copy_(s)
            self._refresh16(params)

    def restore(self, parameters=None):
        """Write the parameters kept by store() back and drop the copy."""
        if self.collected_params is None:
            raise RuntimeError("This ParameterEMA has no `store()`ed weights to `restore()`")
        params = self._get_parameters(parameters)
        with torch.no_grad():
            for c, p in zip(self.collected_params, params):
                p.data.copy_(c)
            self._refresh16(params)
        self.collected_params = None

    @contextlib.contextmanager
    def average_parameters(self, parameters=None):
        """Context manager: the averaged weights inside, the parameters as they were outside (also after an exception).
        torch_ema does it with store() / copy_to() / restore(); here it is swap() twice."""
        params = self._get_parameters(parameters)
        self.swap(params)
        try:
            yield
        finally:
            self.swap(params)

    def to(self, device=None, dtype=None):
        self.shadow_params = [s.to(device=device, dtype=dtype if s.is_floating_point() else None) for s in self.shadow_params]
        if self.collected_params is not None:
            self.collected_params = [c.to(device=device, dtype=dtype if c.is_floating_point() else None)
                                     for c in self.collected_params]

    def reseed(self, parameters=None):
        """Start the average afresh from the current parameters (num_updates back to 0)."""
        params = self._get_parameters(parameters)
        self._check_whole(params)
        with torch.no_grad():
            for s, p in zip(self.shadow_params, params):
                s.copy_(p)
        if self.num_updates is not None:
            self.num_updates = 0
        self.collected_params = None

    def state_dict(self):
        """The dictionary torch_ema writes: the reference's Trainer.load_checkpoint hands it to a torch_ema object."""
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params,
                "collected_params": self.collected_params}

    def load_state_dict(self, state_dict):
        """Inverse of state_dict() (also of torch_ema's).  The shadows are written in place: their addresses do not change."""
        decay = state_dict["decay"]
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        num_updates = state_dict["num_updates"]
        if not (num_updates is None or isinstance(num_updates, int)):
            raise ValueError("ParameterEMA.load_state_dict: invalid num_updates")
        shadows = state_dict["shadow_params"]
        if not isinstance(shadows, (list, tuple)) or not all(torch.is_tensor(t) for t in shadows):
            raise ValueError("ParameterEMA.load_state_dict: shadow_params must be a list of tensors")
        if len(shadows) != len(self.shadow_params):
            raise ValueError(f"ParameterEMA.load_state_dict: {len(shadows)} shadow parameters in the state, "
                             f"{len(self.shadow_params)} parameters here")
        for i, (s, t) in enumerate(zip(self.shadow_params, shadows)):
            if tuple(s.shape) != tuple(t.shape):
                raise ValueError(f"ParameterEMA.load_state_dict: shadow parameter {i} has shape {tuple(t.shape)}, "
                                 f"the parameter {tuple(s.shape)}")
        collected = state_dict.get("collected_params")
        if collected is not None:
            if not isinstance(collected, (list, tuple)) or len(collected) != len(self.shadow_params) or \
                    any(tuple(c.shape) != tuple(s.shape) for c, s in zip(collected, self.shadow_params)):
                raise ValueError("ParameterEMA.load_state_dict: collected_params do not match the parameters")
        self.decay, self.num_updates = decay, num_updates
        with torch.no_grad():
            for s, t in zip(self.shadow_params, shadows):
                s.copy_(t)
        self.collected_params = None if collected is None else \
            [c.detach().clone().to(s.device) for c, s in zip(collected, self.shadow_params)]
