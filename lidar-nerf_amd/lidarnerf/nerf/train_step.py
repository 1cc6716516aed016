"""LiDAR training step: loss of the reference Trainer.train_step (lidarnerf/nerf/utils.py:697-884) and the inner loop
of train_one_epoch (1206-1226): zero_grad -> autocast(render + loss) -> scaled backward -> [DP all-reduce] ->
scaler.step(optimizer) -> scaler.update() -> lr_scheduler.step().  Only the LiDAR branch exists in the reference
path (opt.enable_lidar is forced True, main_lidarnerf.py:229)."""
import contextlib

import torch

from .. import _hip, parallel
from . import captured_step, checkpoint
from .loss import (_CRITERIA, _DEFAULT_OPTIONS, _GRAD_CRITERIA, _SOBEL_X, _SOBEL_Y, LidarLossOptions, _criterion,  # noqa: F401
                   _FusedLidarLoss, _ScaleGrad, fused_lidar_loss, lidar_loss, patch_gradient_loss)  # (callers import them from here)


class LidarTrainer:
    """The hot loop, the checkpoints in the reference Trainer's layout and — `ema_decay` — the exponential moving average
    of the parameters the reference evaluates on (no logging: that is host glue outside the path).

    fused_table_optimizer (default on for fp16 + a fusable field on the GPU): the 13.7 M-parameter hash table — 99.8 %
    of all parameters — leaves torch.optim.Adam / GradScaler and is stepped by ONE kernel (lnh_adam_table_step) that
    reads the fp16 gradient the backward kernels produce and writes the fp32 master table, its moments and the fp16
    copy of the next step.  Same arithmetic as torch's fused Adam, same GradScaler contract (dynamic loss scale, inf/nan
    => the step is skipped for EVERY parameter and the scale backs off); the MLP parameters stay on torch's Adam."""

    def __init__(self, model, lr=1e-2, iters=30000, fp16=True, alpha_d=1000.0, alpha_r=1.0, alpha_i=10.0,
                 alpha_grad=100.0, scale=1.0, world_size=1, render_kwargs=None, fused_table_optimizer=True,
                 mlp_dtype=torch.float16, shard_table_optimizer=False, graph=False, loss_options=None, ema_decay=None,
                 ema_interval=None, nerf_mvl=False, intensity_inv_scale=1.0, fused_points=False):
        # mlp_dtype: the autocast dtype — torch.float16 (the reference's --fp16) or torch.bfloat16 (BASELINE config 5:
        # bf16 MFMA MLPs; the hash table and its gradient stay fp16, so the dynamic loss scale is kept either way)
        # (the backward picks reduce-scatter or all-reduce from the process group, parallel.world_size(): a world_size
        #  argument that disagrees with it would silently run without the exchange and fail later, in gather_table_state)
        if world_size > 1 and parallel.world_size() != world_size:
            raise RuntimeError(f"LidarTrainer(world_size={world_size}) but the initialised process group has "
                               f"{parallel.world_size()} rank(s): call torch.distributed.init_process_group first")
        self.model, self.fp16, self.world, self.amp_dtype = model, fp16, world_size, mlp_dtype
        # the gradient exchange runs with more than one rank — or on a one-rank process group that was asked to exchange
        # all the same (parallel.FORCE_SINGLE_RANK: the way to run the collectives through RCCL on a one-GPU box)
        self.dp = world_size > 1 or parallel.dp_active()
        self.alpha = (alpha_d, alpha_r, alpha_i, alpha_grad)
        self.scale = scale
        # the reference CLI's loss options (LidarLossOptions; None: the defaults).  A frozen value: assign a new one to
        # change them (the captured steps are keyed on it)
        self.loss_options = loss_options if loss_options is not None else LidarLossOptions()
        if not isinstance(self.loss_options, LidarLossOptions):
            raise TypeError(f"LidarTrainer(loss_options=): a LidarLossOptions, not {type(self.loss_options).__name__}")
        self.render_kwargs = render_kwargs or {}
        # evaluation only (eval_step / evaluate): the reference's opt.dataloader == "nerf_mvl" (ground-truth ray-drop -1
        # marks pixels outside the sensor's window) and MAEMeter's intensity_inv_scale (main_lidarnerf.py)
        self.nerf_mvl, self.intensity_inv_scale = bool(nerf_mvl), float(intensity_inv_scale)
        # evaluate(points_intrinsics=): the points meter on the device (metrics.FramePointsEvaluator) instead of
        # metrics.PointsMeter.  An attribute, assignable between evaluations; off keeps every number of PointsMeter bit for bit
        self.fused_points = bool(fused_points)
        # Adam(betas .9/.99, eps 1e-15) and lr * 0.1^(it/iters) (main_lidarnerf.py:389-391, 408-410)
        # get_params returns generators: materialise them; one fused kernel for all parameter groups on the GPU
        params = [dict(g, params=list(g["params"])) for g in model.get_params(lr)]
        # layout of the reference's optimizer (Adam over model.get_params(lr), main_lidarnerf.py:389-391): the order in
        # which its state_dict numbers the parameters — checkpoints are written / read in that layout
        self._ref_layout = [[p for p in g["params"]] for g in params]
        self.epoch, self.stats = 0, {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
        on_gpu = all(p.is_cuda for g in params for p in g["params"])
        self.table, self.sharded = None, False
        self.occupancy = bool(getattr(model, "cuda_ray", False))
        self.update_extra_interval, self.global_step = 16, 0
        if fused_table_optimizer and fp16 and on_gpu and hasattr(model, "fused_spec") and \
                (not self.occupancy or self._ragged_chain(model)):
            try:
                tp = model.fused_spec().table_param
            except AttributeError:
                tp = None
            others = [p for g in params for p in g["params"] if p is not tp]
            # the fused optimizer steps EVERY parameter: the table from its fp16 gradient and the other tensors (the MLP
            # weights: a handful of small fp32 matrices) in the same launch
            if tp is not None and tp.dtype == torch.float32 and tp.is_contiguous() and tp.numel() % 4 == 0 and \
                    len(others) <= _hip.TRAIN_MAX_SMALL and \
                    all(p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda for p in others):
                self.table = tp
                params = [dict(g, params=[p for p in g["params"] if p is not tp]) for g in params]
                self.t_m, self.t_v = torch.zeros_like(tp), torch.zeros_like(tp)
                # every scalar of the optimizer in ONE device buffer (include/lidarnerf_hip.h LNH_TS_*): a captured step
                # needs no host value.  loss_scale / growth_tracker / t_steps are views of it (the names rounds 2-4 used).
                self.opt_state = torch.zeros(_hip.TRAIN_STATE_FLOATS, dtype=torch.float32, device=tp.device)
                self.opt_state[_hip.TS_SCALE] = 65536.0
                self.loss_scale = self.opt_state[_hip.TS_SCALE:_hip.TS_SCALE + 1].view(())
                self.growth_tracker = self.opt_state[_hip.TS_GROWTH:_hip.TS_GROWTH + 1].view(())
                self.t_steps, self.t_flip = [self.opt_state[_hip.TS_T_NEXT:_hip.TS_T_NEXT + 1].view(())] * 2, 0
                self._one = torch.ones((), dtype=torch.float32, device=tp.device)
                self._lr0, self._iters = float(lr), float(iters)
                self.small = others
                self.small_off = [0]
                for p in others:
                    self.small_off.append(self.small_off[-1] + p.numel())
                self.small_m = torch.zeros(max(self.small_off[-1], 1), dtype=torch.float32, device=tp.device)
                self.small_v = torch.zeros_like(self.small_m)
                self._small_stepped = set()  # ids of the small parameters that have taken a step (torch creates state lazily)
                tp._lnh_keep_grad16 = True
                tp._lnh_direct_small_grads = True
                tp._lnh_table16 = tp.detach().to(torch.half).reshape(-1, 2).contiguous()
                tp._lnh_table16_version = tp._version  # fused.table16_of re-casts when the parameter is written elsewhere
                # data parallel, second cut (parallel.py): reduce-scatter of the table gradient, every rank steps 1/N of
                # the rows, all-gather of the fp16 compute copy.  The fp32 master table and the Adam moments of a rank are
                # then current on ITS rows only: gather_table_state() completes them (checkpoints call it).
                self.sharded = bool(shard_table_optimizer and self.dp)
                tp._lnh_shard_optimizer = self.sharded
                tp._lnh_master_stale = False
        params = [g for g in params if len(g["params"])]
        # the reference's groups differ in nothing but their parameter lists (network.py get_params: every group at `lr`):
        # step them as ONE group — torch launches its fused Adam once per group — and keep the reference's grouping for
        # the checkpoint layout only (nerf/checkpoint.py)
        if len(params) > 1 and all({k: v for k, v in g.items() if k != "params"} ==
                                   {k: v for k, v in params[0].items() if k != "params"} for g in params):
            params = [dict(params[0], params=[p for g in params for p in g["params"]])]
        # graph=True: the whole step is captured in a hipGraph per (batch shape, sample capacity) and replayed — what that
        # takes and what it freezes: the docstring of nerf/captured_step.py
        self.graph = bool(graph and self.table is not None and on_gpu and (not self.dp or parallel.backend() == "nccl"))
        if graph and not self.graph:
            raise RuntimeError("LidarTrainer(graph=True): the captured step needs the fused chain with the fused table "
                               "optimizer (fp16, a fusable field on the GPU)" +
                               (f" and, data parallel, the 'nccl' (RCCL) backend — this process group runs "
                                f"'{parallel.backend()}', whose collectives cannot be captured" if self.dp else ""))
        self._graphs, self._graph_warm, self._graph_pool, self.graph_error = {}, set(), None, None
        self._capture_stream, self.capture_ms = None, []
        # With the fused optimizer (self.table is not None) this torch optimizer never steps: it holds the parameter groups
        # the scheduler and the checkpoint layout are written against (lr stays a host number; the kernels form the same
        # schedule on the device from their own step counter).
        self.optimizer = torch.optim.Adam(params, betas=(0.9, 0.99), eps=1e-15, fused=on_gpu)
        if self.table is not None:
            self.optimizer._opt_called = True  # (the scheduler's "step() before optimizer.step()" check: the kernels are the optimizer)
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimizer, lambda it: 0.1 ** min(it / iters, 1))
        self.scaler = torch.amp.GradScaler("cuda", enabled=fp16)
        self.params = [p for g in self.optimizer.param_groups for p in g["params"]]
        # ema_decay (the reference: 0.95, main_lidarnerf.py:431): a ParameterEMA (nerf/ema.py) over model.parameters(), in
        # that order, as nerf/utils.py:619-624 builds torch_ema's.  None (the default): no buffer, no launch, no checkpoint
        # key.  ema_update() is the public call — the reference's cadence is once per epoch, the caller's loop decides;
        # ema_interval=N makes step() call it after every N-th step (after the replay, outside any captured graph).
        self.ema, self.ema_interval = None, None
        if ema_interval is not None:
            if ema_decay is None:
                raise ValueError("LidarTrainer(ema_interval=) needs ema_decay")
            if int(ema_interval) != ema_interval or ema_interval < 1:
                raise ValueError(f"LidarTrainer(ema_interval={ema_interval!r}): a positive number of steps")
            self.ema_interval = int(ema_interval)
        if ema_decay is not None:
            from .ema import ParameterEMA
            self.ema = ParameterEMA(model.parameters(), float(ema_decay))

    @staticmethod
    def _ragged_chain(model):
        """Occupancy-grid sampling renders through the fused ragged chain (nerf/fused.py) when the field has the shapes it is
        built for: the table gradient then arrives in fp16 like the dense chain's; otherwise through the modular density() /
        color() path, where it is a normal .grad and the table stays in torch.optim.Adam."""
        from . import fused
        return bool(getattr(model, "fused_lidar", False)) and fused.ragged_supported(model)

    def loss(self, rays_o, rays_d, images_lidar, patch=(1, 1), grad_scale=None):
        """grad_scale (device scalar): the loss comes back unscaled, its gradient multiplied by it."""
        from . import fused
        ad, ar, ai, ag = self.alpha
        opts = None if self.loss_options.is_default else self.loss_options
        # the default loss with one ray per patch, its gradient pre-scaled (backward starts from ONE): the dense fused chain
        # may form the loss gradient and the compositing adjoint inside its forward tail (fused.TRAIN_TAIL)
        if opts is None and patch[0] <= 1 and grad_scale is not None and images_lidar.is_cuda:
            fused.TRAIN_TAIL = (images_lidar, ad, ar, ai, grad_scale)
        try:
            out = self.model.render(rays_o, rays_d, cal_lidar_color=True, staged=False, perturb=True,
                                    **self.render_kwargs)
        finally:
            fused.TRAIN_TAIL = None
        if out.get("train_tail"):
            # (its gradients are formed already; the same kernel gives the value)
            return fused_lidar_loss(out, images_lidar, ad, ar, ai, value_only=True)
        if out["depth_lidar"].is_cuda and (patch[0] <= 1 or (patch[1] >= 2 and out["depth_lidar"].numel() %
                                                               (patch[0] * patch[1]) == 0)):
            return fused_lidar_loss(out, images_lidar, ad, ar, ai,
                                    None if patch[0] <= 1 else (patch[0], patch[1], self.scale, ag), grad_scale,
                                    options=opts, scale=self.scale)
        loss, pred_depth, gt_depth = lidar_loss(out, images_lidar, ad, ar, ai, options=opts, scale=self.scale)
        if patch[0] > 1:
            loss = loss + patch_gradient_loss(pred_depth, gt_depth, images_lidar[..., 0], patch[0], patch[1],
                                              self.scale, ag, options=opts)
        return loss if grad_scale is None else _ScaleGrad.apply(loss, grad_scale)

    def _forward_backward(self, rays_o, rays_d, images_lidar, patch):
        """Render + loss + backward of one batch with the fused optimizer's conventions: the gradients come out multiplied by
        the CURRENT loss scale — the table's in fp16 (`table._lnh_grad16`), the small tensors' as `.grad` views of one arena.
        Nothing is stepped (tests/test_patch_step_gpu.py compares exactly this state with the oracle)."""
        tp = self.table
        for p in self.small:
            p.grad = None
        tp._lnh_grad16 = None
        tp._lnh_grad_reduced = False
        tp._lnh_grad16_handles = None
        tp._lnh_small_arena = None
        with torch.autocast("cuda", dtype=self.amp_dtype):
            loss = self.loss(rays_o, rays_d, images_lidar, patch, grad_scale=self.loss_scale)
        loss.backward(gradient=self._one)  # (the loss kernel has multiplied its gradients by the loss scale)
        return loss

    def _step_fused_table(self, rays_o, rays_d, images_lidar, patch):
        """One iteration with the fused optimizer: render + loss + backward, (the gradient exchange,) and the optimizer as two
        launches — lnh_train_check (finite check of every gradient, 1 / scale, the learning rate of this step) and
        lnh_train_step (Adam on the table and on the small tensors, GradScaler's skip / scale update, the step counters)."""
        from .fused import table16_of
        tp, st = self.table, self.opt_state
        loss = self._forward_backward(rays_o, rays_d, images_lidar, patch)
        # --- data parallel: the small gradients.  The fused chain leaves all of them in ONE arena (views): that tensor goes
        # on the wire as it is, summed — the division by the world size is folded into 1 / scale like the table's
        div_small, small_handle = 1.0, None
        if self.dp:
            arena = getattr(tp, "_lnh_small_arena", None)
            if arena is not None:
                import torch.distributed as dist
                small_handle = dist.all_reduce(arena, op=dist.ReduceOp.SUM, async_op=True)
                div_small = float(self.world)
            else:
                parallel.allreduce_gradients(self.small, self.world)
        # data parallel: the fp16 table gradient arrives as the sum over ranks; its mean is taken in fp32 by the kernels
        div = float(getattr(tp, "_lnh_grad16_div", 1))
        shards = getattr(tp, "_lnh_grad16_shards", None) if self.sharded else None
        g16 = tp._lnh_grad16
        if g16 is None and not shards:
            raise RuntimeError("fused table optimizer: the backward pass produced no fp16 table gradient "
                               "(render did not go through the fused LiDAR chain)")
        grads = [p.grad for p in self.small]
        for p, g in zip(self.small, grads):
            if g is not None:
                if not (g.dtype == torch.float32 and g.is_contiguous()):
                    raise RuntimeError("fused optimizer: gradients of the small parameters must be contiguous fp32")
                self._small_stepped.add(id(p))
        n_small = len(self.small)
        gp = _hip.ptr_array([None if g is None else g.data_ptr() for g in grads])
        pp = _hip.ptr_array([p.data_ptr() for p in self.small])
        nn_ = _hip.u32_array([p.numel() for p in self.small])
        cast = lambda arr: _hip.C.cast(arr, _hip.C.c_void_p)
        if small_handle is not None:
            small_handle.wait()
        check = lambda ptr, n, first: _hip.call("lnh_train_check", st.data_ptr(), ptr, n, cast(gp), cast(nn_),
                                                n_small if first else 0, div, div_small, self._lr0, self._iters)
        step_args = (cast(pp), cast(gp), cast(nn_), n_small, self.small_m.data_ptr(), self.small_v.data_ptr(), 0.9, 0.99,
                     1e-15, 2.0, 0.5, 2000)
        if shards:
            import torch.distributed as dist
            rank = dist.get_rank()
            for i, (r0, r1, mine, handle, _padded) in enumerate(shards):
                handle.wait()
                rows = parallel.rank_rows(r0, r1, mine.shape[0], rank)[1]
                check(mine.data_ptr() if rows else None, rows * 2, i == 0)
            # every rank has looked at its own rows only: the skip / back-off decision must be the same everywhere (the stamp
            # of a step is the same number on every rank, so MAX keeps it)
            dist.all_reduce(st[_hip.TS_FOUND:_hip.TS_FOUND + 1], op=dist.ReduceOp.MAX)
            shadow = table16_of(tp)  # (re-cast first if somebody wrote the parameter since the last step)
            _hip.call("lnh_train_step", st.data_ptr(), None, None, None, None, None, 0, *step_args)
            self._step_table_shards(shards, shadow)
        else:
            for handle in getattr(tp, "_lnh_grad16_handles", None) or ():
                handle.wait()  # the table windows' all-reduce (left in flight by the backward pass)
            tp._lnh_grad16_handles = None
            check(g16.data_ptr(), g16.numel(), True)
            shadow = table16_of(tp)  # (re-cast first if somebody wrote the parameter since the last step)
            _hip.call("lnh_train_step", st.data_ptr(), tp.data_ptr(), self.t_m.data_ptr(), self.t_v.data_ptr(), g16.data_ptr(),
                      shadow.data_ptr(), tp.numel(), *step_args)
        if not torch.cuda.is_current_stream_capturing():
            self.scheduler.step()  # (host bookkeeping only: the kernels form the schedule from their own counter)
        return loss

    def steps_taken(self):
        """Number of optimizer steps applied so far (skipped steps — inf / nan gradients — do not count).  Synchronises."""
        return int(self.opt_state[_hip.TS_T_NEXT]) if self.table is not None else None

    def _sync_counters(self, steps=None):
        """After a load: the device-side counters follow the host's (scheduler position; optionally the Adam step count)."""
        it = float(self.scheduler.last_epoch)
        self.opt_state[_hip.TS_IT], self.opt_state[_hip.TS_IT_NEXT] = it, it
        # the inf / nan stamp is `it + 1` of the step that saw it and relies on `it` only ever growing: after a rewind a stale
        # stamp would match again when training reaches that iteration (a finite step skipped, the loss scale halved)
        self.opt_state[_hip.TS_FOUND], self.opt_state[_hip.TS_SKIPPED] = 0.0, 0.0
        if steps is not None:
            self.opt_state[_hip.TS_T], self.opt_state[_hip.TS_T_NEXT] = float(steps), float(steps)

    # ---- the captured step (graph=True; nerf/captured_step.py)
    def _graph_capacity(self):
        """Sample capacity of the marcher for a captured step (captured_step.graph_capacity); 0 while there is no mean yet."""
        return captured_step.graph_capacity(self)

    def _step_table_shards(self, shards, shadow):
        """Sharded table optimizer: Adam on this rank's rows of every level window (learning rate, 1 / scale, the skip flag
        and the step counter read from the optimizer's device scalars, which lnh_train_check / lnh_train_step have set), then
        the all-gather of the fp16 compute copy (the only part of the table the next forward pass reads)."""
        import torch.distributed as dist
        tp, st = self.table, self.opt_state
        sp = lambda i: st.data_ptr() + 4 * i
        rank = dist.get_rank()
        flat16, table16 = shadow.view(-1), shadow.view(-1, 2)
        gathers = []
        for r0, r1, mine, _h, padded in shards:
            row0, rows = parallel.rank_rows(r0, r1, mine.shape[0], rank)
            if rows:
                o = row0 * 2  # element offset of the shard in the [rows, 2] table
                _hip.call("lnh_adam_table_step_dlr", tp.data_ptr() + 4 * o, self.t_m.data_ptr() + 4 * o,
                          self.t_v.data_ptr() + 4 * o, mine.data_ptr(), flat16.data_ptr() + 2 * o, rows * 2, sp(_hip.TS_LR), 0.9,
                          0.99, 1e-15, sp(_hip.TS_INV_TABLE), sp(_hip.TS_SKIPPED), sp(_hip.TS_T), sp(_hip.TS_T_NEXT))
            mine16 = torch.zeros_like(mine)
            if rows:
                mine16[:rows] = table16[row0:row0 + rows]
            # (the window's padded gradient buffer has served its purpose: it receives the gathered copy)
            gathers.append((dist.all_gather_into_tensor(padded, mine16, async_op=True), padded, r0, r1))
        for handle, out, r0, r1 in gathers:
            handle.wait()
            table16[r0:r1] = out[:r1 - r0]  # the shards back to back; what lies beyond r1 is padding
        tp._lnh_grad16_shards = None
        # from here on the fp32 master (and the moments) of this rank are current on ITS rows only: whoever reads
        # `embeddings` itself (GridEncoder.forward, grad_total_variation, a state_dict) must gather_table_state() first
        tp._lnh_master_stale = True

    def gather_table_state(self):
        """Sharded table optimizer: complete the fp32 master table and the Adam moments on every rank from their owners
        (checkpoints, evaluation through `embeddings`, a switch back to the replicated optimizer).  Collective."""
        if not self.sharded:
            return
        import torch.distributed as dist
        from .fused import _level_windows
        enc = self.model.fused_spec().grid
        off, world, rank = enc._offsets_host, dist.get_world_size(), dist.get_rank()
        for t in (self.table.data, self.t_m, self.t_v):
            rows = t.view(-1, 2)
            for l0, l1 in _level_windows(enc):
                r0, r1 = int(off[l0]), int(off[l1])
                s = parallel.shard_rows(r1 - r0, world)
                mine = torch.zeros((s, 2), dtype=t.dtype, device=t.device)
                a, n = parallel.rank_rows(r0, r1, s, rank)
                if n:
                    mine[:n] = rows[a:a + n]
                full = torch.empty((world * s, 2), dtype=t.dtype, device=t.device)
                dist.all_gather_into_tensor(full, mine)
                rows[r0:r1] = full[:r1 - r0]
        self.table._lnh_master_stale = False

    # ---- exponential moving average of the parameters (ema_decay; the reference's self.ema, nerf/utils.py:619-624)
    def _require_ema(self, what):
        if self.ema is None:
            raise RuntimeError(f"LidarTrainer.{what}: this trainer keeps no parameter average (construct it with ema_decay=)")

    def ema_update(self):
        """One averaging step (the reference: once per epoch, utils.py:1257-1258).  On the GPU one lnh_ema_update launch on
        the current stream; never from inside a capture.  Sharded table optimizer: COLLECTIVE (gather_table_state: a rank's
        fp32 master is current on its own rows only) — call it on every rank.  Non-sharded data parallel needs no
        communication: every rank holds the same parameters and forms the same average."""
        self._require_ema("ema_update()")
        self.gather_table_state()
        self.ema.update()

    def _ema_swap(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LidarTrainer: the averaged weights cannot be swapped while a stream is capturing")
        self.ema.swap()

    @contextlib.contextmanager
    def ema_weights(self):
        """Context manager: the model carries the averaged weights inside (the reference evaluates on them, utils.py:
        1297-1299 / 1444-1445) and its own again outside, also after an exception.  Each way is ONE lnh_ema_swap launch on
        the current stream that exchanges parameters and shadows in place and, with the fused table optimizer, rewrites the
        persistent fp16 copy of the table in the same pass; inside, fused.table16_of(..., training=False) returns that copy
        instead of re-casting the table per render call.  Nothing moves a version counter or a pointer: the captured steps
        (graph=True) stay valid.  Do not step inside.  Sharded table optimizer: entering is COLLECTIVE (gather_table_state)
        — enter it on every rank."""
        self._require_ema("ema_weights()")
        self.gather_table_state()
        self._ema_swap()
        tp = self.table
        if tp is not None:
            tp._lnh_ema_weights = True
        try:
            yield self.ema
        finally:
            if tp is not None:
                del tp._lnh_ema_weights
            self._ema_swap()

    # ---- evaluation (nerf/evaluate.py; the reference's eval_step / test_step / evaluate_one_epoch, utils.py:886-1009,
    # 1282-1447)
    def eval_step(self, data):
        """The reference's Trainer.eval_step (utils.py:886-977) on one frame: data["rays_o_lidar"] / ["rays_d_lidar"]
        [1, H*W, 3], data["images_lidar"] [1, H, W, 3] on the GPU.  Renders with model.render(cal_lidar_color=True,
        staged=True, perturb=False) under no_grad and the trainer's autocast dtype and render_kwargs, and returns its nine
        values: pred_intensity [1,H,W,1], pred_depth [1,H,W], pred_depth_crop, pred_raydrop [1,H,W,1], gt_intensity
        [1,H,W,1], gt_depth [1,H,W], gt_depth_crop, gt_raydrop [1,H,W,1], loss (0-dim, on the device).  The crops are None
        unless nerf_mvl; with it the intensity images and the crops are [1, crop_h, crop_w(, 1)] — their shape costs this
        method one host read.  Masking, loss: lnh_lidar_eval_frame (include/lidarnerf_hip.h).  The model's mode and weights
        are the caller's (the reference calls it from evaluate_one_epoch); evaluate() is the loop."""
        from . import evaluate
        return evaluate.eval_step(self, data)

    def test_step(self, data, perturb=False):
        """The reference's Trainer.test_step (utils.py:980-1009): data["rays_o_lidar"], ["rays_d_lidar"] [B, H*W, 3],
        ["H_lidar"], ["W_lidar"] -> (pred_raydrop, pred_intensity, pred_depth), [B, H, W] each; intensity and depth are
        multiplied by (pred_raydrop > 0.5) whenever alpha_r > 0 (no "not all zero" exception, no ground truth)."""
        from . import evaluate
        return evaluate.test_step(self, data, perturb)

    def evaluate(self, frames, *, points_intrinsics=None, ema=True, save_dir=None):
        """The reference's evaluate_one_epoch (utils.py:1282-1447) over `frames`, any iterable of eval_step's `data` dicts
        (the loaders of lidarnerf.dataset.range_image yield them), all of one size.  model.eval(); with `ema` and a trainer
        that keeps a parameter average the frames are rendered on the averaged weights (ema_weights(): with the sharded
        table optimizer entering it is COLLECTIVE — call evaluate() on every rank); every frame goes through the render and
        metrics.FrameEvaluator.update (no host read per frame); points_intrinsics=(fov_up, fov) also feeds the masked depth
        of the full frame to metrics.PointsMeter (chamfer distance / F-score; that meter keeps its host read), or on a
        trainer with fused_points=True (constructor argument and attribute; nerf.evaluate.evaluate takes it as a keyword) to
        metrics.FramePointsEvaluator (the same numbers with per-frame means in fp64, no host read per
        frame; a frame with an empty cloud is refused by its measure() at the end of the loop); save_dir
        writes ep<epoch>_<frame>_lidar.npy point clouds through convert.pano_to_lidar (needs points_intrinsics; no PNG
        colour maps).  Appends the mean validation loss to stats["valid_loss"] and, as utils.py:1422-1436 does, the first
        number of the LAST meter to stats["results"]: the chamfer distance with points_intrinsics, the depth RMSE in metres
        without (the depth meter always runs here, so the reference's "no meter: the loss" case does not arise).  Weights
        and the model's train / eval mode are restored also after an exception.  Each rank evaluates the frames it is
        given; nothing is reduced across ranks.  Returns FrameEvaluator.measure()'s dict (+ "points"); its per-frame
        history holds the first 4096 frames, the means every frame.  A frame whose numbers cannot be averaged (NeRF-MVL
        valid pixels that do not fill their rectangle — the reference raises inside eval_step — or a non-finite number) is
        counted on the device whatever its index and refused by measure() at the END of the loop: nothing is appended to
        stats then, but that frame's PointsMeter update and .npy file have already happened."""
        from . import evaluate
        return evaluate.evaluate(self, frames, points_intrinsics=points_intrinsics, ema=ema, save_dir=save_dir,
                                 fused_points=self.fused_points)

    # ---- mesh export (nerf/mesh.py; the reference's save_mesh, utils.py:1011-1040)
    def save_mesh(self, save_path, resolution=256, threshold=10, ema=True):
        """The reference's Trainer.save_mesh: the density on a resolution^3 lattice over model.aabb_infer (model.density
        under no_grad and the trainer's autocast setting, the volume kept on the device), marching cubes at `threshold` on
        the device (csrc/mesh.hip), vertices mapped into the box in float64, a binary PLY at save_path (its directory is
        created).  With `ema` and a trainer that keeps a parameter average the mesh is that of the averaged weights
        (ema_weights(), as evaluate() does).  Parameters, optimizer state, counters and captured steps are left as they
        were.  Not from inside a capture: the two counts are read back once.  Sharded table optimizer: COLLECTIVE
        (gather_table_state) — call it on every rank.  Triangle order and the choice on ambiguous cells are this package's
        own, not PyMCubes' (DESIGN §14).  Returns (n_vertices, n_triangles)."""
        from . import mesh
        return mesh.save_mesh(self, save_path, resolution=resolution, threshold=threshold, ema=ema)

    def mesh_scene(self, resolution=256, threshold=10, ema=True, grid_resolution=None):
        """save_mesh without the file: the same mesh (vertices in world coordinates, equal bit for bit to what read_ply returns
        from save_mesh's file) as a lidarnerf.raycast.RaycastingScene on the device, ready for cast_rays / intersect_lidar /
        raydrop_features (the reference's LidarNVSMeshing, lidarnvs/lidarnvs_meshing.py).  Training state is left as save_mesh
        leaves it.  Not from inside a capture.  Raises on an empty mesh."""
        from . import mesh
        return mesh.mesh_scene(self, resolution=resolution, threshold=threshold, ema=ema, grid_resolution=grid_resolution)

    # ---- what lives outside torch.optim / GradScaler when the table is stepped by the fused kernel
    def table_grad(self):
        """fp32, unscaled gradient of the hash table of the LAST step (the fused path keeps it in fp16 and never sets
        `.grad` on the parameter: code that wants `embeddings.grad` — gradient clipping, `grad_total_variation` — asks
        here).  None before the first step or without the fused table optimizer."""
        g16 = getattr(self.table, "_lnh_grad16", None) if self.table is not None else None
        if g16 is None:
            return None
        for handle in getattr(self.table, "_lnh_grad16_handles", None) or ():
            handle.wait()
        div = float(getattr(self.table, "_lnh_grad16_div", 1))
        # (the scale the backward ran with — the optimizer kernel has already moved loss_scale on growth / backoff steps)
        return g16.float().reshape(self.table.shape) / (self.opt_state[_hip.TS_LAST_SCALE] * div)

    def state_dict(self):
        """Everything a resume needs: torch optimizer / scheduler / scaler state plus — fused table optimizer — the
        table's Adam moments, its device-side step counter and the dynamic loss scale (99.8 % of the optimizer state) and
        — a trainer with ema_decay — the parameter average under "ema" (absent otherwise).
        Sharded table optimizer: COLLECTIVE (gather_table_state) — call it on every rank."""
        self.gather_table_state()
        sd = {"optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
              "scaler": self.scaler.state_dict(), "fused_table": None}
        if self.table is not None:
            sd["fused_table"] = {"exp_avg": self.t_m, "exp_avg_sq": self.t_v, "step": self.t_steps[self.t_flip].clone(),
                                 "loss_scale": self.loss_scale.clone(), "growth_tracker": self.growth_tracker.clone(),
                                 # the small tensors' moments, back to back in the order of self.small
                                 "small_exp_avg": self.small_m, "small_exp_avg_sq": self.small_v,
                                 "small_stepped": [id(p) in self._small_stepped for p in self.small]}
        if self.ema is not None:
            sd["ema"] = self.ema.state_dict()
        return sd

    def load_state_dict(self, sd):
        self.optimizer.load_state_dict(sd["optimizer"])
        captured_step.after_optimizer_load(self)
        self.scheduler.load_state_dict(sd["scheduler"])
        self.scaler.load_state_dict(sd["scaler"])
        ft = sd.get("fused_table")
        if (ft is None) != (self.table is None):
            raise RuntimeError("LidarTrainer.load_state_dict: checkpoint and trainer disagree on the fused table optimizer")
        if ft is not None:
            self.t_m.copy_(ft["exp_avg"])
            self.t_v.copy_(ft["exp_avg_sq"])
            self.loss_scale.copy_(ft["loss_scale"])
            self.growth_tracker.copy_(ft["growth_tracker"])
            if "small_exp_avg" in ft:
                self.small_m.copy_(ft["small_exp_avg"])
                self.small_v.copy_(ft["small_exp_avg_sq"])
                self._small_stepped = {id(p) for p, f in zip(self.small, ft["small_stepped"]) if f}
            self._sync_counters(steps=float(ft["step"]))
        if self.ema is not None and sd.get("ema") is not None:
            self.ema.load_state_dict(sd["ema"])

    # ---- checkpoints in the reference Trainer's format (nerf/checkpoint.py; lidarnerf/nerf/utils.py:1449-1568)
    def save_checkpoint(self, path, full=True, gather=True, ema_model=False):
        """Same dictionary as Trainer.save_checkpoint (utils.py:1449-1480): epoch, global_step, stats, model and — `full`
        — optimizer / lr_scheduler / scaler in the layout the reference's Trainer.load_checkpoint restores (a reference
        run can resume from it and vice versa: the state dict keys of the model are the reference's, see network.py).

        Sharded table optimizer (shard_table_optimizer=True): the master table and the moments live in pieces on the
        ranks, so completing them is a COLLECTIVE.  Two ways to write a checkpoint:
          * call save_checkpoint(path) on EVERY rank — all of them gather, rank 0 alone writes the file (the others
            return the path without touching it); a call on rank 0 only would wait for the others forever;
          * the reference's convention, save on local_rank 0 only (utils.py:1069-1074): call gather_table_state() on every
            rank first, then save_checkpoint(path, gather=False) where the reference saves.  Without the gather that
            raises instead of writing a table with other ranks' stale rows.

        A trainer with ema_decay writes the parameter average under "ema" (`full`; utils.py:1463-1464), in torch_ema's
        state-dict layout.  ema_model=True: "model" is the state dict under the AVERAGED weights (swapped in for the
        state_dict() call and back out) — what the reference's best=True checkpoint holds (utils.py:1492-1504)."""
        return checkpoint.save_checkpoint(self, path, full=full, gather=gather, ema_model=ema_model)

    def load_checkpoint(self, path, model_only=False):
        """Trainer.load_checkpoint (utils.py:1511-1568): a bare state dict or the dictionary above; strict=False.

        A trainer with ema_decay restores the average from the file's "ema" (the reference's rule, utils.py:1538-1539).
        When the file has none — a bare state dict, model_only, a checkpoint written without EMA — the shadows are
        RE-SEEDED from the loaded parameters and num_updates goes back to 0: a deliberate deviation from the reference,
        which would go on averaging from its random initialisation."""
        return checkpoint.load_checkpoint(self, path, model_only=model_only)

    def step(self, rays_o, rays_d, images_lidar, patch=(1, 1)):
        loss = self._step(rays_o, rays_d, images_lidar, patch)
        if self.ema_interval and self.global_step % self.ema_interval == 0:
            self.ema_update()  # (after the replay, outside any captured graph, on the same stream)
        return loss

    def step_sampled(self, sampler):
        """step() on a batch the step draws itself from `sampler` (dataset.sampler.LidarBatchSampler: frame of the epoch,
        random patches, rays and targets in one launch): occupancy update, global_step and the EMA cadence as in step().
        Launch by launch: sampler.draw(), then the step.  graph=True: the sampler's two launches are captured at the head of
        the step's graph and write the graph's own inputs — a replay needs no batch from the host and no copy into the
        graph.  The patch shape of the loss is the sampler's."""
        loss = self._step(None, None, None, sampler.patch, sampler=sampler)
        if self.ema_interval and self.global_step % self.ema_interval == 0:
            self.ema_update()
        return loss

    def train_epoch(self, sampler, steps=None):
        """The reference's train_one_epoch (utils.py:1206-1260) on a LidarBatchSampler: sampler.new_epoch() (a fresh frame
        order), then one step_sampled per frame — or `steps` of them.  The losses are summed on the device and read ONCE
        (the reference reads loss.item() every step); returns their mean, appends it to stats["loss"], bumps `epoch`.  The
        reference's per-epoch EMA update is the caller's (ema_update(), or ema_interval=)."""
        sampler.new_epoch()
        n = len(sampler) if steps is None else int(steps)
        if n <= 0:
            raise ValueError(f"LidarTrainer.train_epoch(steps={steps!r}): a positive number of steps")
        total = None
        for _ in range(n):
            loss = self.step_sampled(sampler).detach().float()
            total = loss if total is None else total + loss
        mean = float(total) / n  # (the one host read of the epoch)
        self.epoch += 1
        self.stats["loss"].append(mean)
        return mean

    def _step(self, rays_o, rays_d, images_lidar, patch, sampler=None):
        if self.occupancy and self.global_step % self.update_extra_interval == 0:
            with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.fp16):
                # refresh the occupancy grid the marcher reads (every 16 steps)
                self.model.update_extra_state(ordered_march=self.render_kwargs.get("ordered_march"))
        self.global_step += 1
        if self.graph:
            if sampler is not None:
                return captured_step.step_graphed(self, sampler.rays_o[None], sampler.rays_d[None], sampler.gt[None], patch,
                                                  sampler=sampler)
            return captured_step.step_graphed(self, rays_o, rays_d, images_lidar, patch)
        if sampler is not None:
            rays_o, rays_d, images_lidar = sampler.draw()
        if self.table is not None:
            return self._step_fused_table(rays_o, rays_d, images_lidar, patch)
        self.optimizer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=self.amp_dtype, enabled=self.fp16):
            loss = self.loss(rays_o, rays_d, images_lidar, patch)
        self.scaler.scale(loss).backward()
        if self.dp:
            parallel.allreduce_gradients(self.params, self.world)
        self.scaler.step(self.optimizer)
        self.scaler.update()
        self.scheduler.step()
        return loss
