"""The captured step of LidarTrainer(graph=True) (fused chain + fused table optimizer): the whole step — (march,) render
chain, loss, backward, (the gradient exchange,) both optimizers, loss-scale update — is captured in a hipGraph per (batch
shape, sample capacity) and replayed (step_graphed).  Built for occupancy-grid sampling; the dense step (no data-dependent sizes
at all) captures the same way and then costs the host 0.05 ms instead of ~0.8 — it is GPU-bound either way on the
fast hosts of this build, a slower host is not (3.42 against 2.21 ms).  The step is ~45 launches over
~0.4 M samples: eager, the host cannot issue them as fast as the GPU retires them (profiles/r04_bench_nerfmvl.json:
1.0 ms of host time per 0.7 ms of kernels).  What a capture freezes — kernel arguments — must not change between
replays, so the learning rate becomes a device scalar (torch's capturable Adam, lnh_adam_table_step_dlr) and the
marcher's sample capacity comes from a ladder of sizes (graph_capacity; the reference sizes it to the running
mean rounded to 128, raymarching.py:223-229: a larger buffer drops fewer rays on overflow, nothing else changes).
Data parallel (round 5): under RCCL (backend "nccl") the collectives of the step — the windowed fp16 all-reduce
or reduce-scatter / all-gather of the table, the MLP gradients, the found-inf MAX — are captured with it, each on
RCCL's own stream inside the graph, so N ranks replay N identical graphs and none of them is host-bound (eight
processes share the 16-CPU quota of a box).  gloo cannot be captured (its collectives synchronise with the host).

Every function takes the trainer; the state (_graphs, _graph_warm, _graph_pool, graph, graph_error, _capture_stream,
capture_ms) stays on it."""
import gc
import math
import os
import time

import torch


# rungs per octave of the captured step's sample-capacity ladder (graph_capacity)
_LADDER_RUNGS_PER_OCTAVE = int(os.environ.get("LNH_GRAPH_LADDER", "8"))


def graph_capacity(trainer):
    """Sample capacity of the marcher for a captured step: the running mean of the recent marches (renderer.py
    update_extra_state) rounded UP to the next of a geometric ladder of capacities (ratio 2^(1/8), multiples of 1024;
    LNH_GRAPH_LADDER = rungs per octave): while the occupancy grid is still settling the mean swings by tens of percent
    from one grid update to the next (measured on the NeRF-MVL-shaped bench: 107 K .. 393 K over 300 steps), and every
    distinct capacity is one capture (0.7 .. 0.9 ms since the trainer captures without emptying the allocator's cache) —
    the ladder has ~15 rungs over that range, each captured once and kept.  On average 4 % of the buffer is padding (zero
    samples the chain runs over; 9 % with the 2^(1/4) ladder of round 4, when a capture cost 70 ms: 0.500 against
    0.516 ms per step at 66 .. 69 samples per ray).  0 while there is no mean yet (the first 16 steps march into N x 1024
    buffers and read the count back)."""
    mc = int(trainer.model.mean_count)
    if mc <= 0:
        return 0
    per = _LADDER_RUNGS_PER_OCTAVE
    rung = math.ceil(per * math.log2(max(mc, 1024) / 1024.0) - 1e-9)
    return int(math.ceil(1024 * 2 ** (rung / per) / 1024.0)) * 1024


def _capture(trainer, rays_o, rays_d, images_lidar, patch, cap, sampler=None):
    """Capture one step on copies of the batch and replay it once.  Returns the entry, or None when the capture or that
    first replay did not go through: graph mode is then off for good and graph_error says why.
    With a `sampler` (dataset.sampler.LidarBatchSampler) the batch tensors only give the shapes: the sampler's two launches
    (draw, cursor advance) are captured at the head of the step and write the graph's own inputs — the capture records them
    without running them, so the first replay below IS this step's draw."""
    model, tp = trainer.model, trainer.table
    if trainer._graph_pool is None:
        # one memory pool for all captured steps: they never run concurrently and none reads what another left
        # behind, so a later capture may reuse what an earlier one freed (and no capture after the largest pays
        # for fresh device allocations)
        trainer._graph_pool = torch.cuda.graph_pool_handle()
    ent = {"rays_o": torch.empty_like(rays_o), "rays_d": torch.empty_like(rays_d),
           "gt": torch.empty_like(images_lidar), "counter": torch.zeros(2, dtype=torch.int32, device=tp.device),
           "graph": torch.cuda.CUDAGraph()}
    if sampler is not None:
        ent["inds"] = torch.empty_like(sampler.inds)
    else:
        for k, src in (("rays_o", rays_o), ("rays_d", rays_d), ("gt", images_lidar)):
            ent[k].copy_(src)
    if trainer.occupancy:
        model._static_march = (ent["counter"], cap - 128)  # (march_rays_train adds its 128-alignment on top)
    try:
        # capture_begin / capture_end by hand: torch.cuda.graph's context manager empties the allocator's cache
        # first (every cached block back to the driver: the workspaces of this step and of the evaluation pass
        # are re-allocated afterwards), which made a capture cost 70-80 ms — 140 steps of the occupancy-grid
        # workload, whose sample capacity moves to a new rung (a new capture) whenever the grid has changed enough
        torch.cuda.synchronize()
        if trainer.dp:
            # Data parallel: ProcessGroupNCCL's watchdog thread keeps every EAGER collective in a list until one of
            # its sweeps (every 100 ms) finds the work's end event complete.  RCCL's stream joins the capture below,
            # and hipEventQuery on an event of a stream that is capturing fails with hipErrorCapturedEvent — in the
            # watchdog thread, which takes the process down ("failed once in a dozen runs" in round 5, 1 of 50 in
            # round 6's loop: the chance that a sweep falls into the 1-2 ms of a capture; with the capture stalled for
            # 300 ms it is every run, profiles/r06_rccl_loop.txt).  The collectives of the eager steps have finished
            # (the synchronize above): give the watchdog two sweeps to drop them, so that it has nothing to poll while
            # this thread captures.  Collectives issued DURING a capture are never put on that list.
            time.sleep(float(os.environ.get("LNH_CAPTURE_DRAIN_MS", "250")) * 1e-3)
        t_cap = time.perf_counter()
        if trainer._capture_stream is None:
            trainer._capture_stream = torch.cuda.Stream()
        # no cyclic garbage collection while the stream captures: what a collection frees is arbitrary (an older trainer's
        # captured graphs, say, kept alive by a traceback), and destroying a graph is a HIP call the capture forbids — the
        # process aborted with the collector running inside this window.  (torch.cuda.graph's context manager collects
        # before it captures; this capture skips that manager for the reason above.)
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(trainer._capture_stream):
                # (a capture that polices every thread of the process would trip over the watchdog's other HIP calls)
                ent["graph"].capture_begin(trainer._graph_pool,
                                           capture_error_mode="thread_local" if trainer.dp else "global")
                try:
                    if sampler is not None:
                        sampler.draw_into(ent["rays_o"], ent["rays_d"], ent["gt"], ent["inds"])
                    ent["loss"] = trainer._step_fused_table(ent["rays_o"], ent["rays_d"], ent["gt"], patch).detach()
                    if os.environ.get("LNH_DEBUG_CAPTURE_STALL_MS"):  # (diagnosis only: widens the window above)
                        time.sleep(float(os.environ["LNH_DEBUG_CAPTURE_STALL_MS"]) * 1e-3)
                finally:
                    ent["graph"].capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        # the gradient and the scale it carries live in THIS graph's buffers: table_grad() must see the ones of
        # the graph that was replayed last, not of the one that was captured last
        ent["g16"] = tp._lnh_grad16
        trainer.capture_ms.append(round((time.perf_counter() - t_cap) * 1e3, 2))  # (host time of this capture)
    except Exception as e:  # noqa: BLE001 — a capture that does not go through must not cost the run
        # (nothing of a captured step has executed: the state is what it was.)  Launch by launch from here on; the
        # reason stays readable (bench.py reports it).
        model._static_march = None
        trainer.graph, trainer.graph_error = False, f"{type(e).__name__}: {e}"
        return None
    finally:
        model._static_march = None
    try:
        ent["graph"].replay()
    except Exception as e:  # noqa: BLE001 — a graph the runtime captured and then refuses to launch (same rule)
        trainer.graph, trainer.graph_error = False, f"replay: {type(e).__name__}: {e}"
        return None
    return ent


def _replayed(trainer, ent):
    """What follows the replay of `ent` on the host: the gradient of this graph, the marcher's counter, the scheduler."""
    model, tp = trainer.model, trainer.table
    tp._lnh_grad16 = ent["g16"]
    if trainer.occupancy:
        model.step_counter[model.local_step % 16].copy_(ent["counter"])
        model.local_step += 1
    trainer.scheduler.step()
    return ent["loss"].clone()  # (the graphs share a pool: the next replay of another one may reuse this memory)


def step_graphed(trainer, rays_o, rays_d, images_lidar, patch, sampler=None):
    """One step of graph mode.  With a `sampler` the batch is the sampler's to draw (the tensors passed are its static
    buffers, read for their shapes only): a step that runs launch by launch draws eagerly first, a captured one draws inside
    its graph — every step draws exactly once."""
    model = trainer.model
    # (the dense step has no sample buffers to size: one graph per batch shape)
    cap = graph_capacity(trainer) if trainer.occupancy else -1
    if cap == 0 or not trainer._graph_warm:
        # eager: no sample mean yet / the very first step (it takes every lazy initialisation — workspaces, kernel
        # attributes, optimizer state — out of the captures that follow).
        # (detached: a caller holding the loss would keep this step's autograd graph — and its AccumulateGrad nodes,
        #  bound to the eager stream — alive into the capture that follows)
        trainer._graph_warm.add("eager")
        model._static_march = None
        if sampler is not None:
            sampler.draw()
        return trainer._step_fused_table(rays_o, rays_d, images_lidar, patch).detach()
    # what a capture bakes in as kernel arguments is part of the key: the loss weights, the scene scale, the render
    # arguments (a change of any of them captures a new step instead of silently replaying the old values)
    # ... and the marcher (NeRFRenderer.ordered_march is an attribute, assignable between steps: a replay never marches the
    # other way).  The capacity stays the last element of an unsampled step's key.
    marcher = ("ordered_march", bool(getattr(model, "ordered_march", False))) if trainer.occupancy else ()
    # ... and which forward tail the dense chain takes (fused.train_tail_enabled: LNH_TRAIN_TAIL, read at every call)
    from .fused import train_tail_enabled
    key = (tuple(rays_o.shape), tuple(images_lidar.shape), tuple(patch), tuple(trainer.alpha), float(trainer.scale),
           tuple(sorted((k, repr(v)) for k, v in trainer.render_kwargs.items())), trainer.loss_options,
           ("train_tail", train_tail_enabled())) + marcher + (cap,)
    if sampler is not None:
        # the draw's kernel arguments (sequence, geometry, seed, stream) join the key; the cursor lives in the sampler, so
        # every graph of the capacity ladder reads and advances the same one
        key += ("sampled",) + sampler.graph_key()
    tp = trainer.table
    if getattr(tp, "_lnh_table16_version", None) != tp._version:
        # somebody wrote the fp32 table through torch since the last step (model.load_state_dict, a manual
        # re-initialisation): a replay never runs table16_of, so the fp16 compute copy is re-cast here — the captured
        # kernels read it in place
        from .fused import table16_of
        table16_of(tp)
    ent = trainer._graphs.get(key)
    if ent is None:
        ent = _capture(trainer, rays_o, rays_d, images_lidar, patch, cap, sampler)
        if ent is None:  # (graph mode is off: this step and every later one launch by launch)
            if sampler is not None:
                sampler.draw()  # (nothing of the failed capture has run: this step has not drawn yet)
            return trainer._step_fused_table(rays_o, rays_d, images_lidar, patch).detach()
        trainer._graphs[key] = ent
    else:
        if sampler is None:
            torch._foreach_copy_([ent["rays_o"], ent["rays_d"], ent["gt"]], [rays_o, rays_d, images_lidar])  # one launch
        ent["graph"].replay()
    return _replayed(trainer, ent)


def drop_graphs(trainer):
    """Forget every captured step: the next step runs launch by launch (taking every lazy initialisation and version
    check with it), the one after is captured afresh."""
    had = bool(trainer._graphs)
    trainer._graphs.clear()
    trainer._graph_warm.clear()
    # the graphs' memory pool goes with them: a pool none of whose graphs is alive any more cannot take a new capture
    # (the allocator asserts on it); the next capture opens a new one, and the blocks of the old one go back to the driver
    trainer._graph_pool = None
    if had and torch.cuda.is_available() and not torch.cuda.is_current_stream_capturing():
        torch.cuda.empty_cache()


def after_optimizer_load(trainer):
    """Graph mode: every captured step is dropped after a load (the next step runs launch by launch and takes the
    version checks and lazy initialisations with it)."""
    if trainer.graph:
        drop_graphs(trainer)
