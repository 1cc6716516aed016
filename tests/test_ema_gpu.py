"""Parameter EMA on the device: lnh_ema_update / lnh_ema_swap through the C ABI against the torch formulation evaluated on
the CPU (bit-identical: three individually rounded IEEE fp32 operations on both sides), and LidarTrainer(ema_decay=) with
the fused table optimizer — the shadows against a host replay, training untouched by updates / swaps / evaluations (launch
by launch and as a captured step), evaluation on the averaged weights, the checkpoint round trip, the sharded optimizer."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
RENDER = dict(num_steps=768, upsample_steps=64)


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _values(n, g):
    """fp32 values of very different magnitude, with denormals and zeros of both signs among them."""
    v = torch.randn(n, generator=g) * 10.0 ** torch.randint(-30, 25, (n,), generator=g).float()
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-45, 1.1754944e-38, -3e-39, 1.0, -1.0, 65504.0, 1e-8, 7e-46, -2.5e24])
    k = min(n, special.numel() * 4)
    if k:
        idx = torch.randperm(n, generator=g)[:k]
        v[idx] = special[torch.arange(k) % special.numel()]
    return v


def _pair(n, g):
    """(shadow, parameter): mostly close to each other (an average follows its parameter), some far apart, some equal."""
    p = _values(n, g)
    s = torch.where(torch.rand(n, generator=g) < 0.7, p * (1 + 0.01 * torch.randn(n, generator=g)), _values(n, g))
    if n:
        s[::7] = p[::7]
    return s.contiguous(), p.contiguous()


_SMALL_SIZES = [1, 3, 5, 7, 129, 1001, 33, 255, 257, 4097, 9, 11, 13, 2049, 15, 17]


def _small_sets(count, g):
    """`count` small tensors of odd sizes as views of one buffer each side, at offsets that are 4-byte aligned only."""
    sizes = _SMALL_SIZES[:count]
    total = sum(sizes) + count + 1
    sbuf, pbuf = _pair(total, g)
    offs, o = [], 1
    for n in sizes:
        offs.append(o)
        o += n + 1
    return sizes, offs, sbuf, pbuf


def _arrays(bufs, sizes, offs):
    from lidarnerf import _hip
    cast = lambda arr: C.cast(arr, C.c_void_p)
    return [cast(_hip.ptr_array([b.data_ptr() + 4 * o for o in offs])) for b in bufs] + [cast(_hip.u32_array(sizes))]


def _ptr(t):
    return t.data_ptr() if t.numel() else None


@pytest.mark.parametrize("n", [0, 1, 3, 4, 1023, (1 << 20) + 2])
def test_ema_update_is_bit_identical_to_the_torch_formula(n):
    from lidarnerf import _hip
    assert _hip.TRAIN_MAX_SMALL == 16 == len(_SMALL_SIZES)
    for n_small in (0, 1, _hip.TRAIN_MAX_SMALL):
        for one_minus_decay in (1 - 2 / 11, 0.05, 0.5):
            g = torch.Generator().manual_seed(1000 * n_small + n % 997)
            s, p = _pair(n, g)
            sizes, offs, sbuf, pbuf = _small_sets(n_small, g)
            want, want_small = s.clone(), sbuf.clone()
            for ws, wp in [(want, p)] + [(want_small[o:o + k], pbuf[o:o + k]) for k, o in zip(sizes, offs)]:
                tmp = ws - wp
                tmp.mul_(one_minus_decay)
                ws.sub_(tmp)
            ds, dp, dsb, dpb = s.cuda(), p.cuda(), sbuf.cuda(), pbuf.cuda()
            sa, pa, na = _arrays((dsb, dpb), sizes, offs)
            _hip.call("lnh_ema_update", _ptr(ds), _ptr(dp), n, sa, pa, na, n_small, one_minus_decay)
            torch.cuda.synchronize()
            tag = (n, n_small, one_minus_decay)
            assert torch.equal(ds.cpu(), want), tag
            assert _same_bits(ds, want), tag                       # (zeros keep their sign, denormals survive)
            assert _same_bits(dsb, want_small), tag                # (the gaps between the small tensors are untouched)
            assert _same_bits(dp, p) and _same_bits(dpb, pbuf), tag  # the parameters are only read
            if n >= 1023:
                assert not _same_bits(ds, s) and int((want.abs() < 1.1754944e-38).logical_and(want != 0).sum()) > 0, tag


@pytest.mark.parametrize("n", [0, 1, 3, 4, 1023, (1 << 20) + 2])
def test_ema_swap_exchanges_and_writes_the_fp16_copy(n):
    from lidarnerf import _hip
    for n_small in (0, 1, _hip.TRAIN_MAX_SMALL):
        for with16 in (True, False):
            g = torch.Generator().manual_seed(77 + n_small + n % 991)
            s, p = _pair(n, g)
            sizes, offs, sbuf, pbuf = _small_sets(n_small, g)
            ds, dp, dsb, dpb = s.cuda(), p.cuda(), sbuf.cuda(), pbuf.cuda()
            junk = torch.full((n,), 3.0, dtype=torch.half, device="cuda")
            d16 = junk.clone()
            pa, sa, na = _arrays((dpb, dsb), sizes, offs)
            args = (_ptr(dp), _ptr(ds), _ptr(d16) if with16 else None, n, pa, sa, na, n_small)
            _hip.call("lnh_ema_swap", *args)
            torch.cuda.synchronize()
            tag = (n, n_small, with16)
            assert _same_bits(dp, s) and _same_bits(ds, p), tag
            assert _same_bits(d16, dp.half() if with16 else junk), tag
            want_pb, want_sb = pbuf.clone(), sbuf.clone()
            for k, o in zip(sizes, offs):
                want_pb[o:o + k], want_sb[o:o + k] = sbuf[o:o + k], pbuf[o:o + k]
            assert _same_bits(dpb, want_pb) and _same_bits(dsb, want_sb), tag
            _hip.call("lnh_ema_swap", *args)  # twice: the identity
            torch.cuda.synchronize()
            assert _same_bits(dp, p) and _same_bits(ds, s) and _same_bits(dpb, pbuf) and _same_bits(dsb, sbuf), tag
            assert _same_bits(d16, p.cuda().half() if with16 else junk), tag


# ---------------------------------------------------------------------------------------------------- the trainer
def _trainer(graph=False, rays=1024, **kw):
    import bench
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bench.build_model(dev)
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph, render_kwargs=RENDER, **kw)
    assert tr.table is not None and tr.graph == graph
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, rays, 0, dev, (1, 1), "analytic") for s in range(8)]
    return tr, model, batches, poses


def _evaluate(model, frame):
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        out = model.render(frame[0], frame[1], cal_lidar_color=True, staged=True, max_ray_batch=512, perturb=False, **RENDER)
    model.train()
    return out["depth_lidar"].float().clone(), out["image_lidar"].float().clone()


def _table_index(model, tp):
    return next(i for i, p in enumerate(model.parameters()) if p is tp)


def _host_replay(want, params, n):
    d = min(0.95, (1 + n) / (10 + n))
    one_minus_decay = 1.0 - d
    for s, p in zip(want, params):
        tmp = s - p
        tmp.mul_(one_minus_decay)
        s.sub_(tmp)


def test_trainer_shadows_match_a_host_replay():
    """12 fused steps with ema_interval=3: the parameters are copied to the host after every step, the update formula is
    replayed there at the update points, and the trainer's shadows carry the same bits."""
    tr, model, batches, _ = _trainer(ema_decay=0.95, ema_interval=3)
    assert len(tr.ema.shadow_params) == len(list(model.parameters()))
    want = [p.detach().cpu().clone() for p in model.parameters()]
    assert all(_same_bits(s, w) for s, w in zip(tr.ema.shadow_params, want))
    torch.manual_seed(11)
    for s in range(12):
        tr.step(*batches[s % 8])
        host = [p.detach().cpu() for p in model.parameters()]
        if (s + 1) % 3 == 0:
            _host_replay(want, host, (s + 1) // 3)
            assert tr.ema.num_updates == (s + 1) // 3
            for i, (sh, w) in enumerate(zip(tr.ema.shadow_params, want)):
                assert _same_bits(sh, w), (s, i)
    assert tr.ema.num_updates == 4
    assert not _same_bits(tr.ema.shadow_params[_table_index(model, tr.table)], tr.table)
    tr.ema_update()  # the public call, outside the interval
    _host_replay(want, [p.detach().cpu() for p in model.parameters()], 5)
    assert all(_same_bits(sh, w) for sh, w in zip(tr.ema.shadow_params, want))


def _train(steps, graph, ema):
    tr, model, batches, poses = _trainer(graph=graph, rays=4096, **(dict(ema_decay=0.95, ema_interval=4) if ema else {}))
    import bench
    frame = bench.make_batch(poses, 0, 1500, 0, tr.table.device)
    torch.manual_seed(11)
    losses, captures_at_first_swap, evals = [], None, []
    for s in range(steps):
        losses.append(tr.step(*batches[s % 8]).detach().clone())
        if ema and s + 1 in (8, 16):
            if captures_at_first_swap is None:
                captures_at_first_swap = (len(tr.capture_ms), len(tr._graphs))
            ptrs = (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version)
            with tr.ema_weights():
                evals.append(_evaluate(model, frame))
            assert ptrs == (tr.table.data_ptr(), tr.table._lnh_table16.data_ptr(), tr.table._version)
            assert tr.table._lnh_table16_version == tr.table._version
    torch.cuda.synchronize()
    state = [tr.table.detach().clone(), tr.table._lnh_table16.clone(), tr.t_m.clone(), tr.t_v.clone(), tr.opt_state.clone()]
    state += [p.detach().clone() for p in tr.small] + [torch.stack(losses)]
    if ema:
        assert tr.ema.num_updates == steps // 4 and len(evals) == 2 and not torch.equal(evals[0][0], evals[1][0])
        if graph:
            # the captured steps survived the swaps: nothing was captured after the first swap, nothing fell back
            assert tr.graph and tr.graph_error is None
            assert captures_at_first_swap == (1, 1) == (len(tr.capture_ms), len(tr._graphs))
    return state


@pytest.mark.parametrize("graph", [False, True])
def test_training_does_not_notice_the_average(graph):
    """24 steps at the benchmark's shape from one seed, with and without ema_decay / ema_interval=4 and two ema_weights()
    blocks holding a staged evaluation: the fp32 table, its fp16 copy, both Adam moments, every MLP matrix, the optimizer's
    scalars and all losses agree bit for bit — launch by launch and as a captured step that is never re-captured."""
    a = _train(24, graph, ema=False)
    b = _train(24, graph, ema=True)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same_bits(x, y), i
    assert torch.isfinite(a[-1]).all() and float(a[4][0]) > 0


def test_evaluation_under_ema_weights():
    import bench
    from lidarnerf.nerf import fused
    tr, model, batches, poses = _trainer(ema_decay=0.95)
    torch.manual_seed(11)
    for s in range(6):
        tr.step(*batches[s % 8])
        if s % 2:
            tr.ema_update()
    tp = tr.table
    frame = bench.make_batch(poses, 0, 1500, 0, tp.device)
    before = _evaluate(model, frame)
    live = [p.detach().clone() for p in model.parameters()]
    shadows = [s.clone() for s in tr.ema.shadow_params]
    assert fused.table16_of(tp, training=False).data_ptr() != tp._lnh_table16.data_ptr()
    with tr.ema_weights():
        assert fused.table16_of(tp, training=False).data_ptr() == tp._lnh_table16.data_ptr()
        assert all(_same_bits(p, s) for p, s in zip(model.parameters(), shadows))
        assert all(_same_bits(s, p) for s, p in zip(tr.ema.shadow_params, live))
        assert _same_bits(tp._lnh_table16, tp.detach().half().reshape(-1, 2))
        inside = _evaluate(model, frame)
    assert fused.table16_of(tp, training=False).data_ptr() != tp._lnh_table16.data_ptr()
    assert all(_same_bits(p, b) for p, b in zip(model.parameters(), live))
    assert all(_same_bits(s, w) for s, w in zip(tr.ema.shadow_params, shadows))
    assert _same_bits(tp._lnh_table16, tp.detach().half().reshape(-1, 2))
    after = _evaluate(model, frame)
    assert all(_same_bits(x, y) for x, y in zip(before, after))
    assert not _same_bits(before[0], inside[0])
    # a second model whose parameters were set to the shadows renders the same bits
    other = bench.build_model(tp.device)
    with torch.no_grad():
        for q, s in zip(other.parameters(), shadows):
            q.copy_(s)
    want = _evaluate(other, frame)
    assert all(_same_bits(x, y) for x, y in zip(inside, want))
    # an exception inside leaves everything as it was, the mark removed
    with pytest.raises(KeyError):
        with tr.ema_weights():
            raise KeyError("inside")
    assert not hasattr(tp, "_lnh_ema_weights") and all(_same_bits(p, b) for p, b in zip(model.parameters(), live))
    # the generic interface of the average takes the same kernels: store / copy_to / restore keep the fp16 copy right
    tr.ema.store()
    tr.ema.copy_to()
    assert _same_bits(tp._lnh_table16, shadows[_table_index(model, tp)].half().reshape(-1, 2))
    tr.ema.restore()
    assert all(_same_bits(p, b) for p, b in zip(model.parameters(), live))
    assert _same_bits(tp._lnh_table16, tp.detach().half().reshape(-1, 2))


def test_checkpoint_round_trip_and_resume(tmp_path):
    """Fused table optimizer on the GPU: "ema" travels with the checkpoint, and a trainer resumed from it continues the
    average with the same bits as the uninterrupted one."""
    tr, model, batches, _ = _trainer(ema_decay=0.95, ema_interval=2)

    def steps(t, lo, hi):
        for s in range(lo, hi):
            torch.manual_seed(100 + s)
            t.step(*batches[s % 8])

    steps(tr, 0, 4)
    path = tr.save_checkpoint(os.path.join(tmp_path, "ema_gpu.pth"))
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck["ema"]) == {"decay", "num_updates", "shadow_params", "collected_params"} and ck["ema"]["num_updates"] == 2
    assert all(_same_bits(a, b) for a, b in zip(ck["ema"]["shadow_params"], [s.cpu() for s in tr.ema.shadow_params]))
    best = torch.load(tr.save_checkpoint(os.path.join(tmp_path, "best.pth"), full=False, ema_model=True),
                      map_location="cpu", weights_only=False)
    ti = _table_index(model, tr.table)
    assert _same_bits(best["model"]["encoder.embeddings"], tr.ema.shadow_params[ti].cpu())
    assert not _same_bits(best["model"]["encoder.embeddings"], tr.table)
    assert _same_bits(tr.table._lnh_table16, tr.table.detach().half().reshape(-1, 2))
    tr2, model2, _, _ = _trainer(ema_decay=0.95, ema_interval=2)
    with torch.no_grad():
        for p in model2.parameters():
            p.add_(0.25)
    tr2.load_checkpoint(path)
    assert tr2.ema.num_updates == 2 and tr2.global_step == 4
    assert all(_same_bits(a, b) for a, b in zip(tr2.ema.shadow_params, tr.ema.shadow_params))
    steps(tr, 4, 8)
    steps(tr2, 4, 8)
    assert tr.ema.num_updates == tr2.ema.num_updates == 4
    for i, (a, b) in enumerate(zip(tr.ema.shadow_params, tr2.ema.shadow_params)):
        assert _same_bits(a, b), i
    for a, b in zip(model.parameters(), model2.parameters()):
        assert _same_bits(a, b)
    assert not _same_bits(tr.ema.shadow_params[ti], ck["ema"]["shadow_params"][ti].cuda())


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return str(port)


def test_sharded_table_optimizer_with_ema_two_ranks():
    """2 ranks (gloo) sharing GPU 0 — tests/ema_dp_worker.py: one step plus ema_update() with the sharded table optimizer
    against the replicated one, then ema_weights() in and out."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LNH_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", _free_port(), os.path.join(root, "tests", "ema_dp_worker.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert out.count("EMA-DP-OK") == 2, out[-3000:]
