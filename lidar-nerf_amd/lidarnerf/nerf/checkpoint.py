"""Checkpoints of the fast trainer in the reference Trainer's format (lidarnerf/nerf/utils.py:1449-1568): optimizer and
scheduler state translated to and from the layout the reference's Adam / LambdaLR over model.get_params(lr) write.
LidarTrainer.save_checkpoint / load_checkpoint call into here; state_dict / load_state_dict, the trainer's own format, stay
on the class."""
import torch

from . import captured_step


def _small_slice(trainer, p):
    """Where the moments of the small parameter `p` lie in the flat small_m / small_v buffers."""
    k = next(i for i, q in enumerate(trainer.small) if q is p)
    return slice(trainer.small_off[k], trainer.small_off[k + 1])


def optimizer_state_ref_layout(trainer):
    """torch.optim.Adam.state_dict() as the reference's optimizer would write it: one entry per parameter of
    model.get_params(lr) in order, the fused table optimizer's moments / step count included."""
    own = trainer.optimizer.state_dict()
    own_ids = {id(p): i for i, p in enumerate(p for g in trainer.optimizer.param_groups for p in g["params"])}
    template = {k: v for k, v in own["param_groups"][0].items() if k != "params"} if own["param_groups"] else {}
    # (graph mode keeps lr in a device scalar: the file carries the number, as the reference's does)
    template = {k: (float(v) if torch.is_tensor(v) and v.dim() == 0 else v) for k, v in template.items()}
    state, groups, idx = {}, [], 0
    for gi, group in enumerate(trainer._ref_layout):
        ids = []
        for p in group:
            if trainer.table is not None and p is trainer.table:
                state[idx] = {"step": trainer.t_steps[trainer.t_flip].detach().clone().float().cpu(),
                              "exp_avg": trainer.t_m.detach().clone(), "exp_avg_sq": trainer.t_v.detach().clone()}
            elif trainer.table is not None and id(p) in trainer._small_stepped:
                # stepped by the fused optimizer: its moments are a slice of the flat buffers, the step count is the
                # table's (one counter for all parameters: a skipped step skips every one of them)
                sl = _small_slice(trainer, p)
                state[idx] = {"step": trainer.t_steps[trainer.t_flip].detach().clone().float().cpu(),
                              "exp_avg": trainer.small_m[sl].detach().clone().view_as(p),
                              "exp_avg_sq": trainer.small_v[sl].detach().clone().view_as(p)}
            elif id(p) in own_ids and own_ids[id(p)] in own["state"]:
                state[idx] = own["state"][own_ids[id(p)]]
            ids.append(idx)
            idx += 1
        g = dict(template)
        g["params"] = ids
        groups.append(g)
    return {"state": state, "param_groups": groups}


def load_optimizer_state_ref_layout(trainer, sd):
    """Inverse of the above.  Returns the Adam step count the file carries for the fused optimizer (None: none, or no fused
    optimizer): load_checkpoint commits it once the scheduler's position is loaded too."""
    own_ids = {id(p): i for i, p in enumerate(p for g in trainer.optimizer.param_groups for p in g["params"])}
    own = trainer.optimizer.state_dict()
    idx, loaded_steps = 0, None
    for group in trainer._ref_layout:
        for p in group:
            st = sd["state"].get(idx)
            if st is not None:
                if trainer.table is not None and p is trainer.table:
                    trainer.t_m.copy_(st["exp_avg"].to(trainer.t_m.device))
                    trainer.t_v.copy_(st["exp_avg_sq"].to(trainer.t_v.device))
                    loaded_steps = float(st["step"])
                elif trainer.table is not None and any(q is p for q in trainer.small):
                    sl = _small_slice(trainer, p)
                    trainer.small_m[sl].copy_(st["exp_avg"].to(trainer.small_m.device).reshape(-1))
                    trainer.small_v[sl].copy_(st["exp_avg_sq"].to(trainer.small_v.device).reshape(-1))
                    trainer._small_stepped.add(id(p))
                    if loaded_steps is None:
                        loaded_steps = float(st["step"])
                elif id(p) in own_ids:
                    own["state"][own_ids[id(p)]] = st
            idx += 1
    # learning rates: the reference's groups that hold parameters stepped here, in order; when they are stepped as
    # one merged group (see __init__) they all carry the same value and the first one is taken
    lr_by_pos = [g.get("lr") for g in sd["param_groups"]]
    lrs = [l for l, grp in zip(lr_by_pos, trainer._ref_layout) if any(id(p) in own_ids for p in grp)]
    if len(own["param_groups"]) == 1:
        lrs = lrs[:1]
    for g, lr in zip(own["param_groups"], lrs):
        if lr is not None:
            g["lr"] = lr
    trainer.optimizer.load_state_dict(own)
    captured_step.after_optimizer_load(trainer)
    return loaded_steps


def own_group_of_ref_group(trainer):
    """For every parameter group of the reference's optimizer: index of the group of trainer.optimizer that steps its
    parameters (the table's group, stepped by the fused kernel, and empty groups follow group 0: every group of
    model.get_params(lr) carries the same lr and the same lambda)."""
    own = {id(p): gi for gi, g in enumerate(trainer.optimizer.param_groups) for p in g["params"]}
    return [next((own[id(p)] for p in grp if id(p) in own), 0) for grp in trainer._ref_layout]


def scheduler_state_ref_layout(trainer):
    """LambdaLR.state_dict() as the reference's scheduler over Adam(model.get_params(lr)) writes it: `base_lrs`,
    `_last_lr` and `lr_lambdas` carry one entry per REFERENCE parameter group (6, or 8 with a background net), not per
    group of the merged optimizer stepped here — a stock scheduler loading the file zips them against its groups."""
    sd = dict(trainer.scheduler.state_dict())
    m = own_group_of_ref_group(trainer)
    for key in ("base_lrs", "_last_lr"):
        if key in sd:
            sd[key] = [float(sd[key][i]) if torch.is_tensor(sd[key][i]) else sd[key][i] for i in m]
    if "lr_lambdas" in sd:
        sd["lr_lambdas"] = [sd["lr_lambdas"][i] for i in m]
    return sd


def load_scheduler_state_ref_layout(trainer, sd):
    """Inverse of the above (also accepts a state written per own group, e.g. by LidarTrainer.state_dict)."""
    sd = dict(sd)
    n_own, m = len(trainer.optimizer.param_groups), own_group_of_ref_group(trainer)
    for key in ("base_lrs", "_last_lr", "lr_lambdas"):
        vals = sd.get(key)
        if vals is None or len(vals) == n_own:
            continue
        if len(vals) != len(m):
            raise RuntimeError(f"lr_scheduler state: {len(vals)} entries in '{key}' for {len(m)} reference parameter "
                               f"groups / {n_own} groups stepped here")
        first = {}
        for ref_i, own_i in enumerate(m):
            first.setdefault(own_i, vals[ref_i])
        sd[key] = [first.get(i, vals[0]) for i in range(n_own)]
    trainer.scheduler.load_state_dict(sd)


def save_checkpoint(trainer, path, full=True, gather=True, ema_model=False):
    """LidarTrainer.save_checkpoint (its docstring is the contract)."""
    if ema_model:
        trainer._require_ema("save_checkpoint(ema_model=True)")
    write = True
    if trainer.sharded:
        import torch.distributed as dist
        if gather:
            trainer.gather_table_state()
            write = dist.get_rank() == 0
        elif getattr(trainer.table, "_lnh_master_stale", False):
            raise RuntimeError("save_checkpoint(gather=False) with the sharded table optimizer: call "
                               "gather_table_state() on every rank first (this rank holds only its own rows of the "
                               "table and the Adam moments)")
    if not write:
        return path
    state = {"epoch": trainer.epoch, "global_step": trainer.global_step, "stats": trainer.stats}
    if full:
        state["optimizer"] = optimizer_state_ref_layout(trainer)
        state["lr_scheduler"] = scheduler_state_ref_layout(trainer)
        if trainer.table is not None:  # the dynamic loss scale lives with the fused table optimizer
            state["scaler"] = {"scale": float(trainer.loss_scale), "growth_factor": 2.0, "backoff_factor": 0.5,
                               "growth_interval": 2000, "_growth_tracker": int(trainer.growth_tracker)}
        else:
            state["scaler"] = trainer.scaler.state_dict()
        if trainer.ema is not None:
            state["ema"] = trainer.ema.state_dict()
    if getattr(trainer.model, "cuda_ray", False):  # a reference loader ignores the extra keys
        state["mean_count"], state["mean_density"] = trainer.model.mean_count, trainer.model.mean_density
        state["iter_density"], state["local_step"] = trainer.model.iter_density, trainer.model.local_step
    if ema_model:
        trainer._ema_swap()
        try:
            # (state_dict() returns views of the parameters: the file must hold the values they have NOW)
            state["model"] = {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}
        finally:
            trainer._ema_swap()
    else:
        state["model"] = trainer.model.state_dict()
    torch.save(state, path)
    return path


def load_checkpoint(trainer, path, model_only=False):
    """LidarTrainer.load_checkpoint (its docstring is the contract)."""
    ck = torch.load(path, map_location=next(trainer.model.parameters()).device, weights_only=False)
    # whatever the file holds, the model is about to change under the captured steps (a bare state dict and
    # model_only=True never reach after_optimizer_load): drop them on every path
    captured_step.drop_graphs(trainer)
    if "model" not in ck:
        trainer.model.load_state_dict(ck)
        if trainer.table is not None:
            trainer.table._lnh_master_stale = False  # a loaded table is whole
        if trainer.ema is not None:
            trainer.ema.reseed()
        return [], []
    missing, unexpected = trainer.model.load_state_dict(ck["model"], strict=False)
    if getattr(trainer.model, "cuda_ray", False):
        for key in ("mean_count", "mean_density", "iter_density", "local_step"):
            if key in ck:  # without them the next 16 grid updates are full sweeps and sample buffers are N * 1024
                setattr(trainer.model, key, ck[key])
    if trainer.table is not None:
        trainer.table._lnh_master_stale = False  # a loaded table is whole
    if trainer.ema is not None:
        if not model_only and ck.get("ema") is not None:
            trainer.ema.load_state_dict(ck["ema"])
        else:
            trainer.ema.reseed()
    if model_only:
        return missing, unexpected
    trainer.stats, trainer.epoch, trainer.global_step = ck["stats"], ck["epoch"], ck["global_step"]
    steps = load_optimizer_state_ref_layout(trainer, ck["optimizer"]) if "optimizer" in ck else None
    if "lr_scheduler" in ck:
        load_scheduler_state_ref_layout(trainer, ck["lr_scheduler"])
    if trainer.table is not None:  # the device-side counters follow what was loaded
        trainer._sync_counters(steps=steps)
    if "scaler" in ck and ck["scaler"]:
        if trainer.table is not None:
            trainer.loss_scale.fill_(float(ck["scaler"]["scale"]))
            trainer.growth_tracker.fill_(int(ck["scaler"].get("_growth_tracker", 0)))
        else:
            trainer.scaler.load_state_dict(ck["scaler"])
    return missing, unexpected
