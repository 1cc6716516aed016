"""Fused LiDAR render step: the whole `NeRFRenderer.run` + `NeRFNetwork.density/color` chain of the reference
(lidarnerf/nerf/renderer.py:99-298, lidarnerf/nerf/network.py:162-237) as 7 kernel launches forward (with the step
prologue) and their mirror image backward, with explicit gradients.

Used by NeRFNetwork.render (both flavours: `network` and the tcnn-shaped `network_tcnn`, through `model.fused_spec()`)
for the configuration the reference trains (`cal_lidar_color=True`, hash-grid L=16 F=2, 64-wide sigma net with one
hidden layer, 64-wide LiDAR colour net with two) under fp16 autocast.  Anything else takes the modular path in
renderer.py / network.py, which computes the same values from the same kernels' unfused forms.

Forward                                                       kernels (liblidarnerf_hip.so)
  wsig16, wcol16 = packed weights; cdir = W0[:, :kd] enc(d)   lnh_lidar_step_prologue (frequency-encoded directions; else
  z = near + (far-near) linspace + perturb   (one torch.rand)   lnh_lidar_pack_weights, the model's direction features +
  x = (clip(o + d z) + b) / 2b                                  lnh_lidar_dir_term, lnh_lidar_coarse_sample_points)
  feat = hashgrid(x)      [16, N(T+t), 2] fp16, row-mapped    lnh_grid_encode_forward_mapped_ex
  h16, sigma = sigma_net(feat)  strided into [N,T+t,*]        lnh_density_mlp_forward
  new_z, z_all, perm = resample(z, sigma); x of the new_z     lnh_lidar_resample_points
  (encode + sigma net for the t new samples, same buffers)
  sigma_m, w = merge + weights                                lnh_lidar_color_composite_forward (T+t > 2048:
  rgb = colour_net(h16[perm], cdir) * (w > 1e-4)                lnh_lidar_merge_weights, lnh_lidar_color_forward,
  ws, depth, image = composite(sigma_m, rgb, z_all)             lnh_lidar_composite_forward)
  (LidarTrainer, default loss: + g_image, g_sigma of the ray   lnh_lidar_color_composite_forward_train: the backward
   in the same launch — TRAIN_TAIL below)                        then skips lnh_lidar_composite_backward)
Backward runs the mirror image over all N(T+t) points at once; the hash-table gradient uses the bucketed
scatter-reduce (no HBM atomics) and, data-parallel, goes on the wire in fp16 window by window.
"""
import os

import numpy as np
import torch
from torch.autograd import Function

from .. import _hip, parallel
from ..gridencoder.grid import _workspace, grid_backward_bucketed


class FieldSpec:
    """What the fused chain needs from a field, independent of how the module stores it (`network.NeRFNetwork` keeps
    nn.Linear stacks + `encoder.embeddings`, `network_tcnn.NeRFNetwork` keeps flat tcnn-style `params` vectors):
    tensors that take part in autograd (possibly views of Parameters) + the per-ray direction features."""

    def __init__(self, grid, table, ws0, ws1, wc0, wc1, wc2, n_dir, dir_features, n_color_mats=3, table_param=None,
                 dir_freq_degree=None):
        self.grid, self.table, self.ws0, self.ws1 = grid, table, ws0, ws1
        self.table_param = table_param if table_param is not None else table  # the Parameter DP bookkeeping marks
        self.wc0, self.wc1, self.wc2, self.n_dir, self.dir_features = wc0, wc1, wc2, n_dir, dir_features
        self.n_color_mats = n_color_mats
        # set when dir_features is the frequency encoder of that degree on raw directions (n_dir = 3 + 6 * degree): the fused
        # chain then forms the features inside the direction-term kernel
        self.dir_freq_degree = dir_freq_degree


def _bucketed_backward_ok(enc):
    """The fused chain's table gradient takes the bucketed backward; tables with more than 64 buckets of 8192 rows per
    level (log2_hashmap_size > 19) are outside its plan (workspace size 0) and must take the modular path instead of
    failing in the middle of backward.  Cached on the encoder."""
    ok = getattr(enc, "_lnh_bucketed_ok", None)
    if ok is None:
        ok = _hip.lib().lnh_grid_backward_workspace_size(enc._offsets_host.data_ptr(), 1024, 3, 2, enc.num_levels,
                                                         enc.log2_scale, enc.base_resolution, enc.gridtype_id, 0,
                                                         _hip.LNH_F16) > 0
        enc._lnh_bucketed_ok = ok
    return ok


def supported(model, cal_lidar_color, num_steps, upsample_steps):
    """True when `model` has exactly the shapes the fused kernels are specialised for."""
    try:
        sp = model.fused_spec()
        enc = sp.grid
        ok = (cal_lidar_color and upsample_steps > 0 and model.bg_radius <= 0
              and enc.input_dim == 3 and enc.num_levels == 16
              and enc.level_dim == 2 and enc.gridtype_id in (0, 2) and not enc.align_corners and enc.interp_id == 0
              and tuple(sp.ws0.shape) == (64, 32) and tuple(sp.ws1.shape) == (16, 64)
              and sp.n_color_mats == 3 and 1 <= sp.n_dir <= 128 and tuple(sp.wc0.shape) == (64, sp.n_dir + 15)
              and tuple(sp.wc1.shape) == (64, 64) and tuple(sp.wc2.shape) == (2, 64)
              and model.geo_feat_dim == 15 and (num_steps + upsample_steps) % 16 == 0
              and sp.table.is_cuda)
        if not ok:
            return False
        _hip.require_gridtype(enc.gridtype_id)  # (gridtype 2 needs a library that knows it: lnh_version >= 101)
        return bool(_bucketed_backward_ok(enc))
    except AttributeError:
        return False


def _grid_bwd_workspace(dev, enc, B):
    """(workspace tensor, bytes at its head the backward wants cleared) for a batch of B points — cached per encoder and B:
    the plan is host arithmetic, but the training step asks for it every step."""
    cache = enc.__dict__.setdefault("_lnh_bwd_ws_plan", {})
    ent = cache.get(B)
    off = enc._offsets_host
    if ent is None:
        L = enc.num_levels
        need = _hip.lib().lnh_grid_backward_workspace_size(off.data_ptr(), B, 3, 2, L, enc.log2_scale, enc.base_resolution,
                                                           enc.gridtype_id, 0, _hip.LNH_F16)
        if len(cache) > 16:
            cache.clear()
        ent = cache[B] = [need, None]
    ws = _workspace(dev, ent[0])
    if ent[1] is None or ent[1][0] != ws.numel():
        clear = _hip.lib().lnh_grid_backward_workspace_clear_bytes(off.data_ptr(), B, 3, 2, enc.num_levels, enc.log2_scale,
                                                                   enc.base_resolution, enc.gridtype_id, 0, 0, _hip.LNH_F16,
                                                                   ws.numel())
        ent[1] = (ws.numel(), int(clear))
    return ws, ent[1][1]


def _grid_bwd(g_feat, x01, g_table16, enc, B, ws=None, flags=0):
    """Table gradient of B points.  ws / flags: the caller has cleared the head of the workspace and / or the gradient table
    itself (lnh_grid_encode_backward_ws_ex: LNH_BWD_WS_CLEARED, LNH_BWD_TABLE_ZERO)."""
    if ws is None:
        ws, _ = _grid_bwd_workspace(g_feat.device, enc, B)
    grid_backward_bucketed(g_feat, x01, enc._offsets_host, g_table16, enc.log2_scale, enc.base_resolution, enc.gridtype_id,
                           0, 0, ws, flags=flags, tag=B)


# Data parallel: level windows of the table gradient.  The scatter pass of the backward runs once for all levels
# (lnh_grid_encode_backward_ws_begin); the reduce pass runs per window (_finish), and a window's rows are final as soon as its
# reduce has run, so its collective (fp16, RCCL's own stream) overlaps with the reduce of the next window.  What a window
# costs in compute, measured on one MI355X with the exchange a no-op (bench.py --dp-windows, 4096 rays, ms per step / backward
# us), round 4 — after the reduce pass stopped being as slow as its slowest bucket (rows of the dense levels dealt to 64
# buckets):   no windows 2.149 / 854    1 window 2.154 / 855    2 (0,10,16) 2.192 / 889    3 (0,8,12,16) 2.198 / 890
#             4 (0,7,10,13,16) 2.270 / 957    6 2.412 / 1093
# (round 3: 1 window 2.309 / 1013, 2 -> 2.498 / 1196, 3 -> 2.529 / 1221, 4 -> 2.603 / 1291; round 2 cut the SCATTER pass
# into windows as well: 2.683 / 1362.)  Three windows cost what two cost and cut the table into thirds by rows (39 % / 31 % / 31 %):
# only the last third's exchange has nothing left to hide behind, instead of 46 % with two.  Which count wins in the end
# depends on the all-reduce time, which no box of this build could measure (LNH_DP_WINDOWS overrides the cut for that).
_DP_LEVEL_WINDOWS = ((0, 8), (8, 12), (12, 16))
if os.environ.get("LNH_DP_WINDOWS"):  # developer override for A/B runs: "0,10,16" = two windows
    _c = [int(v) for v in os.environ["LNH_DP_WINDOWS"].split(",")]
    # (must be the same on every rank: the shard layout follows the windows)
    if len(_c) < 2 or _c[0] != 0 or _c[-1] != 16 or any(b <= a for a, b in zip(_c[:-1], _c[1:])):
        raise ValueError(f"LNH_DP_WINDOWS={os.environ['LNH_DP_WINDOWS']!r}: need increasing level cuts from 0 to 16, "
                         "e.g. '0,10,16'")
    _DP_LEVEL_WINDOWS = tuple(zip(_c[:-1], _c[1:]))
FORCE_DP_WINDOWS = False  # bench.py --dp-windows: take the windowed backward on one GPU too (the exchange is a no-op)


def _level_windows(enc):
    """The level windows [l0, l1) in which the table gradient of `enc` is reduced, exchanged and sharded."""
    return _DP_LEVEL_WINDOWS if enc.num_levels == 16 else ((0, enc.num_levels),)


def _grid_bwd_windows(g_feat, x01, g_table16, enc, B, ws=None, flags=0):
    """The table-gradient backward as a generator over level windows: `lnh_grid_encode_backward_ws_begin` once (everything
    but the last reduce pass: the scatter pass stays in ONE piece — cut into level windows it costs 0.33 ms more per 3.4 M
    points, profiles/r03_bench_dpwindows*.json of the first cut), then `..._finish` per window; yields (l0, l1) when the rows
    of that window are final, so that the caller can hand them to a collective while the next window is being reduced."""
    if ws is None:
        ws, _ = _grid_bwd_workspace(g_feat.device, enc, B)
    args = (g_feat, x01, enc._offsets_host, g_table16, enc.log2_scale, enc.base_resolution, enc.gridtype_id, 0, 0, ws)
    grid_backward_bucketed(*args, split=1, flags=flags, timer="lnh_grid_encode_backward_ws_begin", tag=B)
    for window in _level_windows(enc):
        grid_backward_bucketed(*args, window=window, split=2, flags=flags, timer="lnh_grid_encode_backward_ws_finish")
        yield window


def _allreduce_windows(windows, g_table16, enc, table_param):
    """parallel.allreduce_half_table on the table rows of each level window, as `windows` hands them out (a generator does
    its own work in between).  Returns the handles to wait on."""
    off = enc._offsets_host
    handles = []
    for l0, l1 in windows:
        h = parallel.allreduce_half_table(g_table16[int(off[l0]):int(off[l1])], table_param)
        if h is not None:
            handles.append(h)
    return handles


def _grid_bwd_overlapped(g_feat, x01, g_table16, enc, B, table_param, ws=None, flags=0):
    """_grid_bwd + parallel.allreduce_half_table, pipelined over level windows.  Returns the handles to wait on."""
    return _allreduce_windows(_grid_bwd_windows(g_feat, x01, g_table16, enc, B, ws, flags), g_table16, enc, table_param)


def _grid_bwd_sharded(g_feat, x01, enc, B, table_param):
    """Data parallel, sharded table optimizer (parallel.py "second cut"): per level window, the finished rows are copied
    into a buffer padded to world * shard rows and REDUCE-SCATTERED (fp16, SUM) — each rank keeps only its rows.
    Returns [(r0, r1, shard tensor [s, 2] fp16, handle, padded buffer)] per window of table rows [r0, r1): this rank's shard
    holds the rows parallel.rank_rows(r0, r1, s, rank).  Pipelined like the all-reduce: the collective of a window
    runs behind the reduce pass of the following windows."""
    import torch.distributed as dist
    off = enc._offsets_host
    world = dist.get_world_size()
    g_table16 = torch.zeros((int(off[-1]), 2), dtype=torch.half, device=g_feat.device)
    shards = []
    for l0, l1 in _grid_bwd_windows(g_feat, x01, g_table16, enc, B):
        r0, r1 = int(off[l0]), int(off[l1])
        s = parallel.shard_rows(r1 - r0, world)
        padded = torch.zeros((world * s, 2), dtype=torch.half, device=g_feat.device)
        padded[:r1 - r0] = g_table16[r0:r1]
        mine = torch.empty((s, 2), dtype=torch.half, device=g_feat.device)
        h = parallel.reduce_scatter_half(padded, mine)
        shards.append((r0, r1, mine, h, padded))
    table_param._lnh_grad_reduced = True
    return shards


def table16_of(param, embeddings=None, training=True):
    """fp16 compute copy of the hash table.  With the fused table optimizer (train_step.LidarTrainer) the copy is a
    persistent shadow that the optimizer kernel rewrites together with the fp32 master; it is tied to the master's
    torch version counter, so a write to the parameter through torch (load_state_dict, parallel.broadcast_parameters, a
    manual re-initialisation under no_grad) is noticed here and the shadow is re-cast.  Writes through `.data` (torch_ema's
    copy_to / restore) do not move the version counter: evaluation (`training=False`) therefore never trusts the shadow
    and casts the parameter as it is — 82 MB of traffic per render call, noise next to the render itself — except inside
    LidarTrainer.ema_weights(), whose swap kernel writes parameter and shadow together and marks the parameter.  Without a
    shadow the table is cast per call (the autocast rule of grid.py:54-57)."""
    src = param if embeddings is None else embeddings
    shadow = getattr(param, "_lnh_table16", None)
    if shadow is not None and not training and getattr(param, "_lnh_ema_weights", False):
        # inside LidarTrainer.ema_weights(): lnh_ema_swap has written the shadow together with the parameter
        return shadow
    if shadow is not None and getattr(param, "_lnh_shard_optimizer", False):
        # sharded table optimizer: the fp32 master of this rank is current on its own rows only; the all-gathered shadow
        # IS the table (LidarTrainer.gather_table_state() completes the master for checkpoints).  A write to the parameter
        # through torch (load_state_dict, broadcast) moves its version counter — the optimizer kernel and the gather do not —
        # and then the parameter is whole and newer: re-cast.
        if getattr(param, "_lnh_table16_version", None) != param._version:
            if getattr(param, "_lnh_master_stale", False):
                # an in-place write that moved the version counter while only this rank's rows of the master are current:
                # re-casting would overwrite the other ranks' rows of the shadow with stale values
                raise RuntimeError("the fp32 hash table was written through torch while the sharded table optimizer holds "
                                   "only this rank's rows of it: call LidarTrainer.gather_table_state() (every rank) "
                                   "before modifying `embeddings`, or load through LidarTrainer.load_checkpoint")
            shadow.copy_(param.detach().reshape(shadow.shape))
            param._lnh_table16_version = param._version
        return shadow
    if shadow is None or not training:
        return src.detach().to(torch.half).contiguous()
    if getattr(param, "_lnh_table16_version", None) != param._version:
        shadow.copy_(param.detach().reshape(shadow.shape))
        param._lnh_table16_version = param._version
    return shadow


def _no_autocast(fn):
    """The kernel chain manages precision itself: run the glue ops (casts, the tiny per-ray GEMMs) with autocast off,
    otherwise fp32 operands of a matmul silently become fp16 tensors handed to kernels that expect fp32."""
    def wrapped(*args, **kwargs):
        with torch.autocast("cuda", enabled=False):
            return fn(*args, **kwargs)
    return wrapped


_SAMPLE_DIST = {}


def _sample_dist(N, value, dev):
    """[N] fp32 tensor filled with `value` — the same every step, so it is kept instead of re-filled (read-only)."""
    if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        # (a captured step keeps the POINTER: never hand it a tensor this cache may drop later)
        return torch.full((N,), value, dtype=torch.float32, device=dev)
    key = (N, value, str(dev))
    t = _SAMPLE_DIST.get(key)
    if t is None:
        if len(_SAMPLE_DIST) > 16:
            _SAMPLE_DIST.clear()
        t = _SAMPLE_DIST[key] = torch.full((N,), value, dtype=torch.float32, device=dev)
    return t


# The five matrices of a field, packed for the kernels (element type mdt: torch.half, or torch.bfloat16 for the bf16-operand
# build of the kernels, config 5 — hash features stay fp16 either way):
#   wsig16 = [ws0 [64, 32] | ws1 [16, 64]]
#   wcol16 = [(0 | wc0[:, kd:kd+15]) [64, 16] | wc1 [64, 64] | wc2 padded to 16 rows [16, 64]]
# The direction columns wc0[:, :kd] act once per RAY (cdir), so a sample's colour input is its own 16-wide sigma-net row.
# The arena of the small gradients (fp32) is [g_wcol | g_wsig | g_wc0 [64, kd + 15]], the first two laid out like the vectors.
_N_WSIG = 64 * 32 + 16 * 64
_N_WCOL = 64 * 16 + 64 * 64 + 16 * 64


def _weight_buffers(small, mdt, dev):
    """(mats, wsig16, wcol16): the fp32 master matrices `small` = (ws0, ws1, wc0, wc1, wc2) as the kernels take them
    (possibly strided views of flat parameter vectors) and the two packed vectors, still empty."""
    mats = [m.detach() if m.dtype == torch.float32 and m.stride(-1) == 1 else m.detach().float().contiguous() for m in small]
    return mats, torch.empty(_N_WSIG, dtype=mdt, device=dev), torch.empty(_N_WCOL, dtype=mdt, device=dev)


def _pack_weights(small, kd, mdt, dev):
    """_weight_buffers, packed: one launch."""
    mats, wsig16, wcol16 = _weight_buffers(small, mdt, dev)
    _hip.call("lnh_lidar_pack_weights" + _hip.mlp_suffix(mdt), mats[0].data_ptr(), mats[0].stride(0), mats[1].data_ptr(),
              mats[1].stride(0), mats[2].data_ptr(), mats[2].stride(0), kd, mats[3].data_ptr(), mats[3].stride(0),
              mats[4].data_ptr(), mats[4].stride(0), wsig16.data_ptr(), wcol16.data_ptr())
    return mats, wsig16, wcol16


def _dir_term_freq(rays_d, spec, wc0, mdt):
    """(enc_d16 [N, kd], cdir [N, 64]) of raw directions: the frequency encoder of `spec`, rounded to the MLP element type,
    and the per-ray direction term of the colour head's first layer (wc0: its entry of `mats`) — one launch."""
    N, dev = rays_d.shape[0], rays_d.device
    enc_d16 = torch.empty((N, spec.n_dir), dtype=torch.float32, device=dev)
    cdir = torch.empty((N, 64), dtype=torch.float32, device=dev)
    _hip.call("lnh_lidar_dir_term_freq" + _hip.mlp_suffix(mdt), rays_d.data_ptr(), int(spec.dir_freq_degree), wc0.data_ptr(),
              wc0.stride(0), N, enc_d16.data_ptr(), cdir.data_ptr())
    return enc_d16, cdir


def _small_param_state(small):
    """(dtypes, the five small matrices as the Parameters they are (network.NeRFNetwork) — or None when the field hands out
    views of flat parameter vectors (network_tcnn): LidarTrainer takes their gradients straight from the backward's arena
    then)."""
    direct = all(isinstance(w, torch.nn.Parameter) and w.dtype == torch.float32 and w.is_contiguous() for w in small)
    return tuple(w.dtype for w in small), small if direct else None


def _small_grad_arena(kd, dev):
    """One fp32 tensor for all gradients of the small matrices, UNCLEARED (the caller clears it in its one zero_regions
    launch), and views of it: (arena, g_wcol, g_wsig, g_w0g [64, 16] — the geo-feature columns of wc0 as the colour
    backward accumulates them —, g_small = the gradients of (ws0, ws1, wc0, wc1, wc2))."""
    arena = torch.empty(_N_WCOL + _N_WSIG + 64 * (kd + 15), dtype=torch.float32, device=dev)
    g_wcol, g_wsig = arena[:_N_WCOL], arena[_N_WCOL:_N_WCOL + _N_WSIG]
    g_small = (g_wsig[:64 * 32].view(64, 32), g_wsig[64 * 32:].view(16, 64), arena[_N_WCOL + _N_WSIG:].view(64, kd + 15),
               g_wcol[64 * 16:-16 * 64].view(64, 64), g_wcol[-16 * 64:].view(16, 64)[:2])
    return arena, g_wcol, g_wsig, g_wcol[:64 * 16].view(64, 16), g_small


def _hand_over_small(table_param, small_params, arena, g_small, dtypes):
    """The five entries of a backward's return tuple for the small matrices."""
    if small_params is not None and getattr(table_param, "_lnh_direct_small_grads", False):
        # LidarTrainer's fused optimizer: the gradients are handed over as views of the arena (autograd's AccumulateGrad
        # would copy each view into a tensor of its own: five launches), and the arena goes on the wire as ONE tensor
        for p_, g_ in zip(small_params, g_small):
            p_.grad = g_
        table_param._lnh_small_arena = arena
        return (None,) * 5
    return tuple(g_.to(dt_) for g_, dt_ in zip(g_small, dtypes))


def _hand_over_table(table_param, g_table16, master_dtype, handles=None):
    """What a backward returns for the hash table, given its fp16 gradient (data parallel: the SUM over ranks; None with
    the sharded optimizer, which has its rows in `_lnh_grad16_shards`) and the collectives still in flight on it."""
    world = parallel.world_size()
    if getattr(table_param, "_lnh_keep_grad16", False):
        # the fused table optimizer consumes the fp16 gradient directly: no fp32 copy, no .grad on the table; it divides
        # by `_lnh_grad16_div` in fp32.  It is the only consumer and waits right before its kernels (train_step.py), so the
        # last window's bytes travel under the MLP gradients' all-reduce and the loss-scale bookkeeping instead of being
        # waited for here, inside backward
        if handles is not None:
            table_param._lnh_grad16_handles = handles
        table_param._lnh_grad16, table_param._lnh_grad16_div = g_table16, world
        return None
    for handle in handles or ():
        handle.wait()
    g_table = g_table16.to(master_dtype)
    if world > 1:
        g_table.div_(world)  # sum over ranks -> mean, after the widening
    return g_table


def _ragged_field(xyzs, rays, M, bound, enc, table16, wsig16, wcol16, cdir, mdt, x01, feat, h16, sigma, rgb):
    """The field on the first M rows of the marcher's samples, into the caller's buffers (at least M rows each): grid
    coordinates x01, hash features feat [L, M, 2], sigma-net rows h16 [M, 16] and densities sigma [M], colours rgb [M, 2]
    of the rows a ray of the table `rays` owns (the others keep what the buffer held)."""
    sfx, L = _hip.mlp_suffix(mdt), enc.num_levels
    _hip.call("lnh_ragged_points", xyzs.data_ptr(), bound, M, x01.data_ptr())
    _hip.call("lnh_grid_encode_forward", x01.data_ptr(), table16.data_ptr(), enc._offsets_host.data_ptr(), feat.data_ptr(),
              M, 3, 2, L, enc.log2_scale, enc.base_resolution, None, enc.gridtype_id, 0, 0, _hip.LNH_F16, tag=M)
    _hip.call("lnh_density_mlp_forward" + sfx, feat.data_ptr(), wsig16.data_ptr(), M, M, M, 0, 0, h16.data_ptr(),
              sigma.data_ptr())
    # colour head, one wave per ray of the marcher's table (round 5; before: a [M, 96] input assembled per sample, the
    # generic 96 -> 64 -> 64 -> 16 MLP kernel and a sigmoid pass)
    _hip.call("lnh_ragged_color_forward" + sfx, h16.data_ptr(), rays.data_ptr(), cdir.data_ptr(), wcol16.data_ptr(),
              rays.shape[0], M, rgb.data_ptr())


# The training forward tail.  Under the default loss with one ray per patch, d loss / d (depth, image) of a ray is a closed
# form of that ray's own outputs, so the forward tail can go on to the compositing adjoint of the ray from what its forward
# walk left in LDS (lnh_lidar_color_composite_forward_train) and the backward pass starts at the colour head;
# sigma_m and rgb, which only the compositing backward read, are then never written.  The loss is the
# trainer's, so LidarTrainer.loss offers what the kernel needs — (gt [N, 3], alpha_d, alpha_r, alpha_i, grad_scale device
# scalar) — in TRAIN_TAIL around its render call; render_lidar takes the offer when the model is training and the samples
# fit the fused tail, and says so in its result ("train_tail": the gradients of depth_lidar / image_lidar that reach the
# node are then IGNORED — the caller must not differentiate anything else through them).  LNH_TRAIN_TAIL=0 (read at every
# call: A/B runs, tests) keeps the three-launch chain forward tail -> lnh_lidar_loss -> lnh_lidar_composite_backward.
TRAIN_TAIL = None


def train_tail_enabled():
    return os.environ.get("LNH_TRAIN_TAIL", "1") != "0"


class FusedLidarRender(Function):
    @staticmethod
    @_no_autocast
    def forward(ctx, rays_o, rays_d, noise, u, embeddings, ws0, ws1, wc0, wc1, wc2, model, density_scale, spec, mdt, near,
                far, T, tail=None):
        # noise: [N*T] uniforms of the stratified perturbation, or None (evaluation)
        # mdt: element type of everything MLP-side (packed weights, sigma-net rows, their gradients)
        sfx = _hip.mlp_suffix(mdt)
        enc = spec.grid
        kd = spec.n_dir
        dev = rays_o.device
        N = rays_o.shape[0]
        t_new = u.shape[1]
        Ttot = T + t_new
        bound = float(model.bound)
        aabb = (model.aabb_train if model.training else model.aabb_infer).float().contiguous()
        # sample_dist = (fars - nears) / T with the fp32 roundings of renderer.py:129-156, formed on the host
        near32 = np.float32(model.min_near_lidar)
        sd = _sample_dist(N, float((np.float32(near32 * np.float32(81.0)) - near32) / np.float32(T)), dev)

        # fp16 copy of the table: maintained by the fused table optimizer when there is one (train_step.LidarTrainer),
        # otherwise cast here (the autocast rule of grid.py:54-57)
        table16 = table16_of(spec.table_param, embeddings, model.training)
        small = (ws0, ws1, wc0, wc1, wc2)
        # direction features [N, kd] (constant along a ray), rounded to the MLP element type (what the MLP would see), and
        # the per-ray direction term of the colour head's first layer
        enc_d16 = torch.empty((N, kd), dtype=torch.float32, device=dev)
        cdir = torch.empty((N, 64), dtype=torch.float32, device=dev)
        z = torch.empty((N, T), dtype=torch.float32, device=dev)
        x01 = torch.empty((N * Ttot, 3), dtype=torch.float32, device=dev)
        deg = spec.dir_freq_degree
        if deg is not None and 3 + 6 * deg == kd:
            # weight packing + direction term (frequency encoder folded in) + the coarse pass (stratified depths and their
            # grid coordinates) in ONE launch
            mats, wsig16, wcol16 = _weight_buffers(small, mdt, dev)
            _hip.call("lnh_lidar_step_prologue" + sfx, mats[0].data_ptr(), mats[0].stride(0), mats[1].data_ptr(),
                      mats[1].stride(0), mats[2].data_ptr(), mats[2].stride(0), int(deg), mats[3].data_ptr(), mats[3].stride(0),
                      mats[4].data_ptr(), mats[4].stride(0), wsig16.data_ptr(), wcol16.data_ptr(),
                      None if noise is None else noise.data_ptr(), rays_o.data_ptr(), rays_d.data_ptr(), aabb.data_ptr(), bound,
                      N, T, Ttot, float(near), float(far), z.data_ptr(), x01.data_ptr(), enc_d16.data_ptr(), cdir.data_ptr())
        else:
            mats, wsig16, wcol16 = _pack_weights(small, kd, mdt, dev)
            enc_d = spec.dir_features(rays_d).contiguous()
            _hip.call("lnh_lidar_dir_term" + sfx, enc_d.data_ptr(), mats[2].data_ptr(), mats[2].stride(0), N, kd,
                      enc_d16.data_ptr(), cdir.data_ptr())
            # coarse pass: the stratified depths and their grid coordinates in one launch
            _hip.call("lnh_lidar_coarse_sample_points", None if noise is None else noise.data_ptr(), rays_o.data_ptr(),
                      rays_d.data_ptr(), aabb.data_ptr(), bound, N, T, Ttot, float(near), float(far), z.data_ptr(),
                      x01.data_ptr())

        h16 = torch.empty((N * Ttot, 16), dtype=mdt, device=dev)
        sigma_pt = torch.empty((N, Ttot), dtype=torch.float32, device=dev)
        # coarse and importance samples of a ray live side by side (slots 0..T-1 | T..T+t-1) in ONE set of buffers, so
        # the backward pass is a single launch chain over all N*(T+t) points
        B_all = N * Ttot
        L = enc.num_levels
        feat = torch.empty((L, B_all, 2), dtype=torch.half, device=dev)

        def density(Tc, off):  # (the prologue / coarse / resample kernel has written the coordinates of these samples)
            B = N * Tc
            _hip.call("lnh_grid_encode_forward_mapped_ex", x01.data_ptr(), table16.data_ptr(),
                      enc._offsets_host.data_ptr(), feat.data_ptr(), B, Tc, Ttot, off, B_all, 2, L, enc.log2_scale,
                      enc.base_resolution, enc.gridtype_id, _hip.LNH_F16, tag=B, timer="lnh_grid_encode_forward_mapped")
            _hip.call("lnh_density_mlp_forward" + sfx, feat.data_ptr(), wsig16.data_ptr(), B, Tc, Ttot, off, B_all,
                      h16.data_ptr(), sigma_pt.data_ptr())

        density(T, 0)
        new_z = torch.empty((N, t_new), dtype=torch.float32, device=dev)
        z_all = torch.empty((N, Ttot), dtype=torch.float32, device=dev)
        perm = torch.empty((N, Ttot), dtype=torch.int32, device=dev)
        # (stage-1 densities = the first T columns of the [N, T+t] buffer: read in place, row stride T+t)
        # ... and the grid coordinates of the new samples are written by the same kernel
        _hip.call("lnh_lidar_resample_points", z.data_ptr(), sigma_pt.data_ptr(), Ttot, sd.data_ptr(), u.data_ptr(), N, T,
                  t_new, float(density_scale), new_z.data_ptr(), z_all.data_ptr(), perm.data_ptr(), rays_o.data_ptr(),
                  rays_d.data_ptr(), aabb.data_ptr(), bound, x01.data_ptr())
        density(t_new, T)
        if CAPTURE is not None:
            CAPTURE.update(z=z, new_z=new_z, z_all=z_all, perm=perm)

        weights = torch.empty((N, Ttot), dtype=torch.float32, device=dev)
        if tail is None:  # (the training forward tail keeps both in LDS: nothing else reads them)
            sigma_m = torch.empty((N, Ttot), dtype=torch.float32, device=dev)
            rgb = torch.empty((N, Ttot, 2), dtype=torch.float32, device=dev)
        ws = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty((N, 2), dtype=torch.float32, device=dev)
        g_sigma = g_image = None
        if tail is not None:
            # ... and the loss gradient + compositing adjoint of every ray behind its forward, in the same launch
            gt, ad, ar, ai, grad_scale = tail
            g_sigma = torch.empty((N, Ttot), dtype=torch.float32, device=dev)
            g_image = torch.empty((N, 2), dtype=torch.float32, device=dev)
            _hip.call("lnh_lidar_color_composite_forward_train" + sfx, z_all.data_ptr(), sigma_pt.data_ptr(), perm.data_ptr(),
                      sd.data_ptr(), h16.data_ptr(), cdir.data_ptr(), wcol16.data_ptr(), N, Ttot, float(density_scale),
                      gt.data_ptr(), float(ad), float(ar), float(ai), None if grad_scale is None else grad_scale.data_ptr(),
                      weights.data_ptr(), ws.data_ptr(), depth.data_ptr(), image.data_ptr(), g_sigma.data_ptr(),
                      g_image.data_ptr(), timer="lnh_lidar_color_composite_forward" + sfx)
        elif Ttot <= 2048:
            # merged densities + weights, colour head, compositing sums: one launch, one wave per ray
            _hip.call("lnh_lidar_color_composite_forward" + sfx, z_all.data_ptr(), sigma_pt.data_ptr(), perm.data_ptr(),
                      sd.data_ptr(), h16.data_ptr(), cdir.data_ptr(), wcol16.data_ptr(), N, Ttot, float(density_scale),
                      sigma_m.data_ptr(), weights.data_ptr(), rgb.data_ptr(), ws.data_ptr(), depth.data_ptr(),
                      image.data_ptr())
        else:
            _hip.call("lnh_lidar_merge_weights", z_all.data_ptr(), sigma_pt.data_ptr(), perm.data_ptr(), sd.data_ptr(), N,
                      Ttot, float(density_scale), sigma_m.data_ptr(), weights.data_ptr())
            _hip.call("lnh_lidar_color_forward" + sfx, h16.data_ptr(), perm.data_ptr(), weights.data_ptr(),
                      cdir.data_ptr(), wcol16.data_ptr(), N, Ttot, rgb.data_ptr())
            _hip.call("lnh_lidar_composite_forward", z_all.data_ptr(), sigma_m.data_ptr(), rgb.data_ptr(), sd.data_ptr(),
                      N, Ttot, 2, float(density_scale), None, ws.data_ptr(), depth.data_ptr(), image.data_ptr())

        if tail is not None:  # (the backward does not need z_all either: it goes back to the allocator here)
            ctx.save_for_backward(x01, feat, h16, perm, weights, g_sigma, g_image, cdir, enc_d16, wsig16, wcol16)
        else:
            ctx.save_for_backward(x01, feat, h16, perm, weights, z_all, sigma_m, rgb, sd, cdir, enc_d16, wsig16, wcol16)
        ctx.train_tail = tail is not None
        ctx.dims, ctx.density_scale, ctx.enc = (N, T, t_new), density_scale, enc
        ctx.table_param, ctx.mdt, ctx.table_dtype = spec.table_param, mdt, embeddings.dtype
        ctx.small_dtypes, ctx.small_params = _small_param_state(small)
        ctx.mark_non_differentiable(weights, z_all)
        # outputs the loss does not use (weights_sum in the LiDAR loss) arrive as None instead of a zero tensor filled
        # for the occasion; the compositing backward takes a null pointer for them
        ctx.set_materialize_grads(False)
        return ws, depth, image, weights, z_all

    @staticmethod
    @_no_autocast
    def backward(ctx, g_ws, g_depth, g_image, _gw, _gz):
        (N, T, t_new), ds = ctx.dims, ctx.density_scale
        enc, table_param = ctx.enc, ctx.table_param
        mdt, sfx = ctx.mdt, _hip.mlp_suffix(ctx.mdt)
        Ttot = T + t_new
        if ctx.train_tail:
            # the forward tail has formed the loss gradient and the compositing adjoint of every ray: straight to the colour head
            x01, feat, h16, perm, weights, g_sigma, g_image, cdir, enc_d16, wsig16, wcol16 = ctx.saved_tensors
            dev = h16.device
        else:
            x01, feat, h16, perm, weights, z_all, sigma_m, rgb, sd, cdir, enc_d16, wsig16, wcol16 = ctx.saved_tensors
            dev = h16.device
            g_ws, g_depth, g_image = (None if g is None else g.contiguous().float() for g in (g_ws, g_depth, g_image))
            ptr = lambda t: None if t is None else t.data_ptr()

            g_sigma = torch.empty((N, Ttot), dtype=torch.float32, device=dev)
            # d loss / d rgb = weights (x) d loss / d image is formed inside the colour backward: the compositing backward
            # writes the density gradient only (grad_rgb = NULL)
            _hip.call("lnh_lidar_composite_backward", ptr(g_ws), ptr(g_depth), ptr(g_image),
                      z_all.data_ptr(), sigma_m.data_ptr(), rgb.data_ptr(), sd.data_ptr(), N, Ttot, 2, float(ds),
                      g_sigma.data_ptr(), None)
            if g_image is None:
                g_image = torch.zeros((N, 2), dtype=torch.float32, device=dev)

        g_h16 = torch.empty((N * Ttot, 16), dtype=mdt, device=dev)
        wws = _hip.wgrad_ws(dev)  # scratch of the fixed-order weight-gradient sums (one per device and stream, kept)
        kd = enc_d16.shape[1]
        # every gradient that is ACCUMULATED into (the small matrices' by the fixed-order sums, the table's by the reduce pass) is cleared
        # by one launch: the arena of all small gradients and — unless the sharded backward brings its own — the fp16 table
        arena, g_wcol, g_wsig, g_w0g, g_small = _small_grad_arena(kd, dev)
        sharded = parallel.dp_active() and getattr(table_param, "_lnh_shard_optimizer", False)
        g_table16 = None if sharded else torch.empty((int(enc._offsets_host[-1]), 2), dtype=torch.half, device=dev)
        # ... and the cursors at the head of the table backward's workspace (its own clear launch is then skipped)
        bwd_ws, bwd_clear = _grid_bwd_workspace(dev, enc, N * Ttot)
        bwd_flags = 0 if sharded else (_hip.LNH_BWD_TABLE_ZERO | (_hip.LNH_BWD_WS_CLEARED if bwd_clear else 0))
        _hip.zero_regions((arena, g_table16, None if sharded or not bwd_clear else bwd_ws[:bwd_clear]))
        ray_sum = torch.empty((N, 64), dtype=torch.float32, device=dev)
        _hip.call("lnh_lidar_color_backward_image" + sfx, g_image.data_ptr(), g_sigma.data_ptr(), h16.data_ptr(), perm.data_ptr(),
                  weights.data_ptr(), cdir.data_ptr(), wcol16.data_ptr(), N, Ttot, g_h16.data_ptr(), g_wcol.data_ptr(),
                  ray_sum.data_ptr(), *wws)
        # the whole gradient of the colour head's first matrix in one launch: direction columns = S^T enc(d), geo-feature
        # columns copied out of the packed [64, 16] block the colour backward accumulated
        _hip.call("lnh_lidar_dir_term_backward", ray_sum.data_ptr(), enc_d16.data_ptr(), N, kd, g_w0g.data_ptr(),
                  g_small[2].data_ptr(), kd + 15, *wws)
        # (ahead of the sigma net's backward, which still adds to g_wsig: what is handed over of an fp32 matrix is a view)
        g_small = _hand_over_small(table_param, ctx.small_params, arena, g_small, ctx.small_dtypes)

        B_all = N * Ttot
        g_feat = torch.empty((enc.num_levels, B_all, 2), dtype=torch.half, device=dev)
        _hip.call("lnh_density_mlp_backward" + sfx, g_h16.data_ptr(), feat.data_ptr(), wsig16.data_ptr(), B_all, Ttot, Ttot, 0,
                  g_feat.data_ptr(), g_wsig.data_ptr(), *wws)
        handles = None
        if sharded:
            # data parallel, sharded table optimizer: reduce-scatter per window; the trainer steps this rank's rows
            table_param._lnh_grad16_shards = _grid_bwd_sharded(g_feat, x01, enc, B_all, table_param)
        elif parallel.dp_active() or FORCE_DP_WINDOWS:
            # data parallel: the table gradient goes on the wire as fp16, window by window, behind the kernels of the
            # following windows
            handles = _grid_bwd_overlapped(g_feat, x01, g_table16, enc, B_all, table_param, bwd_ws, bwd_flags)
        else:
            _grid_bwd(g_feat, x01, g_table16, enc, B_all, bwd_ws, bwd_flags)
        g_table = _hand_over_table(table_param, g_table16, ctx.table_dtype, handles)
        return (None, None, None, None, g_table) + g_small + (None,) * 8


MASK_STATS = None  # bench.py: set to a list to collect, per render call, the fraction of samples with weight > 1e-4
CAPTURE = None  # parity tests: set to a dict to receive the sample depths (z, new_z, z_all, perm) of the next render call


def render_lidar(model, rays_o, rays_d, num_steps, upsample_steps, perturb, noise=None, u=None):
    """Drop-in for NeRFRenderer.run(cal_lidar_color=True) on a supported NeRFNetwork.  `noise` [N, num_steps] / `u`
    [N, upsample_steps] in [0, 1) replace the random draws (perturbation / sample_pdf), as in NeRFRenderer.run."""
    prefix = rays_o.shape[:-1]
    rays_o = rays_o.contiguous().view(-1, 3).float()
    rays_d = rays_d.contiguous().view(-1, 3).float()
    N, dev = rays_o.shape[0], rays_o.device
    # near = min_near_lidar, far = 81 * near: hard-coded 1 m .. 81 m in scene units (renderer.py:129-138); the fp32
    # products are formed exactly as the tensor code of the reference forms them
    near = torch.tensor(float(model.min_near_lidar), dtype=torch.float32)
    far = near * 81.0
    # one random draw serves the stratified perturbation (first N*num_steps values) and, in training mode, the
    # importance-sampling positions u (the rest)
    n_noise = N * num_steps if perturb and noise is None else 0
    n_u = N * upsample_steps if model.training and u is None else 0
    rnd = torch.rand(n_noise + n_u, device=dev) if n_noise + n_u else None
    if not perturb:
        noise = None
    elif noise is None:
        noise = rnd[:n_noise]
    else:
        noise = noise.to(dev).float().reshape(N * num_steps).contiguous()
    if u is not None:
        u = u.to(dev).float().reshape(N, upsample_steps).contiguous()
    elif model.training:
        u = rnd[n_noise:].view(N, upsample_steps)
    else:
        u = torch.linspace(0.5 / upsample_steps, 1.0 - 0.5 / upsample_steps, upsample_steps,
                           device=dev).expand(N, upsample_steps).contiguous()
    sp = model.fused_spec()
    from ..ffmlp.ffmlp import mlp_dtype
    # the trainer's offer of a training forward tail (TRAIN_TAIL above): taken for a training render of these very rays
    # whose samples fit the fused tail, by a library that has the entry point
    tail = TRAIN_TAIL
    if tail is not None and not (model.training and torch.is_grad_enabled() and num_steps + upsample_steps <= 2048
                                 and train_tail_enabled() and tail[0].numel() == 3 * N and tail[0].is_cuda):
        tail = None
    if tail is not None:
        _hip.require_symbols(("lnh_lidar_color_composite_forward_train" + _hip.mlp_suffix(mlp_dtype()),),
                             "the training forward tail (LNH_TRAIN_TAIL=0 keeps the three-launch chain)")
        tail = (tail[0].reshape(N, 3).float().contiguous(),) + tuple(tail[1:])
    ws, depth, image, weights, _ = FusedLidarRender.apply(rays_o, rays_d, noise, u, sp.table, sp.ws0, sp.ws1, sp.wc0,
                                                          sp.wc1, sp.wc2, model, model.density_scale, sp, mlp_dtype(),
                                                          float(near), float(far), num_steps, tail)
    if MASK_STATS is not None:
        MASK_STATS.append((weights > 1e-4).float().mean())
    out = {"depth_lidar": depth.view(*prefix), "image_lidar": image.view(*prefix, 2), "weights_sum_lidar": ws}
    if tail is not None:
        out["train_tail"] = True
    return out


# ------------------------------------------------------------------------------------------------ occupancy-grid chain
class FusedLidarRagged(Function):
    """The occupancy-grid render step (BASELINE config 4; renderer.run_cuda) as one autograd node over the marcher's ragged
    samples: hash-grid encode -> sigma net -> LiDAR colour head -> ragged compositing, and the mirror image backward, on the
    same kernels as the dense chain.  What the modular path does through four autograd nodes, a torch.cat of [M, 90] colour
    inputs in fp32 and per-module casts, runs here as ~12 launches forward / ~12 backward; the hash-table gradient comes out
    of the bucketed scatter-reduce in fp16 and feeds the fused table optimizer (LidarTrainer) like the dense chain's.

    Differences to the dense chain that are properties of the path, not of this implementation: every marched sample lies in
    an occupied cell, so the colour head runs on ALL of them (no weight mask); a ray owns `rays[i, 2]` consecutive samples
    from `rays[i, 1]` on instead of a row of T, so the colour kernels walk the marcher's ray table (one wave per ray group,
    lnh_ragged_color_forward / _backward: the direction term once per ray, K = 16 per sample — round 5; rounds 3-4 assembled
    a [M, 96] input per sample for the generic MLP kernel)."""

    @staticmethod
    @_no_autocast
    def forward(ctx, xyzs, dirs, deltas, rays, rays_o, rays_d, embeddings, ws0, ws1, wc0, wc1, wc2, model, spec, mdt,
                T_thresh):
        enc = spec.grid
        dev = xyzs.device
        M, N, L = xyzs.shape[0], rays.shape[0], enc.num_levels
        kd, ds = spec.n_dir, float(model.density_scale)
        small = (ws0, ws1, wc0, wc1, wc2)
        ctx.meta = (enc, spec.table_param, mdt, float(T_thresh), kd, ds, embeddings.dtype)
        ctx.small_dtypes, ctx.small_params = _small_param_state(small)
        ctx.empty = M == 0
        ctx.set_materialize_grads(False)
        if M == 0:
            # The marcher found no sample (every ray misses the occupied cells).  The node still exists: its outputs are
            # zeros CONNECTED to the graph, and its backward hands out zero gradients and takes part in the gradient
            # exchange — under data parallel a rank that skipped the table all-reduce would leave the others waiting.
            ctx.shapes = tuple(w.shape for w in small)
            z = torch.zeros(N, dtype=torch.float32, device=dev)
            return z, z.clone(), torch.zeros((N, 2), dtype=torch.float32, device=dev)
        table16 = table16_of(spec.table_param, embeddings, model.training)
        mats, wsig16, wcol16 = _pack_weights(small, kd, mdt, dev)
        enc_d16, cdir = _dir_term_freq(rays_d, spec, mats[2], mdt)
        x01 = torch.empty((M, 3), dtype=torch.float32, device=dev)
        feat = torch.empty((L, M, 2), dtype=torch.half, device=dev)
        h16 = torch.empty((M, 16), dtype=mdt, device=dev)
        sigma = torch.empty(M, dtype=torch.float32, device=dev)
        # (colour rows no ray owns stay 0.)  run_cuda hands over rows its prologue launch has already cleared
        rgb = getattr(model, "_lnh_rgb_rows", None)
        model._lnh_rgb_rows = None
        if rgb is None or rgb.shape != (M, 2) or rgb.device != dev or rgb.dtype != torch.float32:
            rgb = torch.zeros((M, 2), dtype=torch.float32, device=dev)
        _ragged_field(xyzs, rays, M, float(model.bound), enc, table16, wsig16, wcol16, cdir, mdt, x01, feat, h16, sigma, rgb)
        sig_s = sigma * ds if ds != 1.0 else sigma
        ws = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty((N, 2), dtype=torch.float32, device=dev)
        _hip.call("lnh_lidar_composite_rays_train_forward", sig_s.data_ptr(), rgb.data_ptr(), deltas.data_ptr(),
                  xyzs.data_ptr(), rays_o.data_ptr(), rays_d.data_ptr(), rays.data_ptr(), M, N, 2, float(T_thresh),
                  ws.data_ptr(), depth.data_ptr(), image.data_ptr())
        ctx.save_for_backward(x01, feat, h16, sig_s, cdir, enc_d16, rgb, deltas, xyzs, rays_o, rays_d, rays, ws, depth, image,
                              wsig16, wcol16)
        return ws, depth, image

    @staticmethod
    @_no_autocast
    def backward(ctx, g_ws, g_depth, g_image):
        enc, table_param, mdt, T_thresh, kd, ds, table_dtype = ctx.meta
        if ctx.empty:  # no sample: zero gradients, but the same collectives as every other rank
            dev = table_param.device
            g_table16 = torch.zeros((int(enc._offsets_host[-1]), 2), dtype=torch.half, device=dev)
            if parallel.dp_active():
                for handle in _allreduce_windows(_level_windows(enc), g_table16, enc, table_param):
                    handle.wait()
            g_table = _hand_over_table(table_param, g_table16, table_dtype)
            zw = tuple(torch.zeros(sh, dtype=dt, device=dev) for sh, dt in zip(ctx.shapes, ctx.small_dtypes))
            return (None, None, None, None, None, None, g_table) + zw + (None, None, None, None)
        (x01, feat, h16, sig_s, cdir, enc_d16, rgb, deltas, xyzs, rays_o, rays_d, rays, ws, depth, image, wsig16,
         wcol16) = ctx.saved_tensors
        sfx = _hip.mlp_suffix(mdt)
        dev = x01.device
        M, N, L = x01.shape[0], rays.shape[0], enc.num_levels
        zN = lambda g, shape: torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else g.contiguous().float()
        g_ws, g_depth, g_image = zN(g_ws, (N,)), zN(g_depth, (N,)), zN(g_image, (N, 2))
        # every buffer that is accumulated into or only partly written — both compositing gradients, the sigma-net rows'
        # gradient (rows no ray owns), the per-ray sums, the small matrices' gradients, the fp16 table gradient, the cursors
        # of the table backward — cleared by ONE launch
        gsf = torch.empty(M * 3, dtype=torch.float32, device=dev)
        arena, g_wcol, g_wsig, g_w0g, g_small = _small_grad_arena(kd, dev)
        g_table16 = torch.empty((int(enc._offsets_host[-1]), 2), dtype=torch.half, device=dev)
        g_h16 = torch.empty((M, 16), dtype=mdt, device=dev)
        ray_sum = torch.empty((N, 64), dtype=torch.float32, device=dev)
        bwd_ws, bwd_clear = _grid_bwd_workspace(dev, enc, M)
        bwd_flags = _hip.LNH_BWD_TABLE_ZERO | (_hip.LNH_BWD_WS_CLEARED if bwd_clear else 0)
        _hip.zero_regions((gsf, arena, g_table16, g_h16, ray_sum, bwd_ws[:bwd_clear] if bwd_clear else None))
        gs, gf = gsf[:M], gsf[M:].view(M, 2)
        _hip.call("lnh_lidar_composite_rays_train_backward", g_ws.data_ptr(), g_depth.data_ptr(), g_image.data_ptr(),
                  sig_s.data_ptr(), rgb.data_ptr(), deltas.data_ptr(), xyzs.data_ptr(), rays_o.data_ptr(),
                  rays_d.data_ptr(), rays.data_ptr(), ws.data_ptr(), depth.data_ptr(), image.data_ptr(), M, N, 2,
                  T_thresh, gs.data_ptr(), gf.data_ptr())
        wws = _hip.wgrad_ws(dev)
        # colour head backward ray by ray: sigmoid, the three layers, all weight gradients, the sigma-net rows' gradient
        # (col 0 = the density gradient through trunc_exp) and the per-ray sum for the direction columns — one launch
        _hip.call("lnh_ragged_color_backward" + sfx, gf.data_ptr(), gs.data_ptr(), ds, h16.data_ptr(), rays.data_ptr(),
                  cdir.data_ptr(), wcol16.data_ptr(), N, M, g_h16.data_ptr(), g_wcol.data_ptr(), ray_sum.data_ptr(), *wws)
        _hip.call("lnh_lidar_dir_term_backward", ray_sum.data_ptr(), enc_d16.data_ptr(), N, kd, g_w0g.data_ptr(),
                  g_small[2].data_ptr(), kd + 15, *wws)
        g_feat = torch.empty((L, M, 2), dtype=torch.half, device=dev)
        _hip.call("lnh_density_mlp_backward" + sfx, g_h16.data_ptr(), feat.data_ptr(), wsig16.data_ptr(), M, M, M, 0,
                  g_feat.data_ptr(), g_wsig.data_ptr(), *wws)
        if parallel.dp_active():
            for handle in _grid_bwd_overlapped(g_feat, x01, g_table16, enc, M, table_param, bwd_ws, bwd_flags):
                handle.wait()
        else:
            _grid_bwd(g_feat, x01, g_table16, enc, M, bwd_ws, bwd_flags)
        g_table = _hand_over_table(table_param, g_table16, table_dtype)
        g_small = _hand_over_small(table_param, ctx.small_params, arena, g_small, ctx.small_dtypes)
        return (None, None, None, None, None, None, g_table) + g_small + (None, None, None, None)


def ragged_supported(model):
    """The occupancy-grid chain needs the same field shapes as the dense chain (and the in-kernel frequency encoder)."""
    try:
        sp = model.fused_spec()
    except AttributeError:
        return False
    # gridtype 0 only: the tcnn-shaped field renders without cuda_ray (as the reference's -L run does), and this chain is
    # not verified on tiny-cuda-nn's lattice (gridtype 2) — such a model takes the modular occupancy path (the grid
    # encoder's own HIP kernels, which serve every gridtype) instead
    return supported(model, True, 16, 16) and sp.grid.gridtype_id == 0 and sp.dir_freq_degree is not None \
        and 3 + 6 * sp.dir_freq_degree == sp.n_dir and sp.n_dir + 15 <= 96


def render_lidar_ragged(model, xyzs, dirs, deltas, rays, rays_o, rays_d, T_thresh):
    """Field + compositing of renderer.run_cuda on the marcher's samples -> (weights_sum [N], depth [N], image [N, 2])."""
    from ..ffmlp.ffmlp import mlp_dtype
    sp = model.fused_spec()
    return FusedLidarRagged.apply(xyzs.contiguous(), dirs.contiguous(), deltas.contiguous(), rays.contiguous(),
                                  rays_o.contiguous(), rays_d.contiguous(), sp.table, sp.ws0, sp.ws1, sp.wc0, sp.wc1, sp.wc2,
                                  model, sp, mlp_dtype(), T_thresh)


class RaggedEvalField:
    """The field half of FusedLidarRagged.forward for the alive-ray evaluation loop (renderer.run_cuda_alive), no autograd:
    what does not change between the rounds of a call — the fp16 table, the packed weights, the per-ray direction term —
    is made once, the per-sample buffers are allocated once for `rows` samples and reused; a round is one _ragged_field on
    the marcher's table — the very function the training chain calls, so a sample's sigma and colour carry the same bits on
    both paths."""

    def __init__(self, model, rays_d, rows):
        from ..ffmlp.ffmlp import mlp_dtype
        self._setup(model, rays_d.contiguous(), int(rows), mlp_dtype())  # (the MLP build follows the caller's autocast dtype)

    @_no_autocast
    def _setup(self, model, rays_d, rows, mdt):
        sp = model.fused_spec()
        self.mdt, self.enc = mdt, sp.grid
        self.bound, self.ds = float(model.bound), float(model.density_scale)
        dev, L = rays_d.device, sp.grid.num_levels
        self.table16 = table16_of(sp.table_param, sp.table, False)
        mats, self.wsig16, self.wcol16 = _pack_weights((sp.ws0, sp.ws1, sp.wc0, sp.wc1, sp.wc2), sp.n_dir, mdt, dev)
        _, self.cdir = _dir_term_freq(rays_d, sp, mats[2], mdt)
        self.N, self.rows = rays_d.shape[0], rows
        self.x01 = torch.empty(rows * 3, dtype=torch.float32, device=dev)
        self.feat = torch.empty(L * rows * 2, dtype=torch.half, device=dev)
        self.h16 = torch.empty(rows * 16, dtype=mdt, device=dev)
        self.sigma = torch.empty(rows, dtype=torch.float32, device=dev)
        self.rgb = torch.empty(rows * 2, dtype=torch.float32, device=dev)

    @_no_autocast
    def __call__(self, xyzs, rays, M):
        """(sigma [M] with density_scale applied, rgb [M, 2]) of the first M rows of xyzs; rgb rows no ray of the table owns
        keep stale values (the compositor reads owned rows only)."""
        if M > self.rows or rays.shape[0] != self.N:
            raise RuntimeError("RaggedEvalField: more samples than the buffers were sized for, or another ray table")
        _ragged_field(xyzs, rays, M, self.bound, self.enc, self.table16, self.wsig16, self.wcol16, self.cdir, self.mdt,
                      self.x01, self.feat, self.h16, self.sigma, self.rgb)
        sigma = self.sigma[:M]
        return (sigma * self.ds if self.ds != 1.0 else sigma), self.rgb[:M * 2].view(M, 2)
