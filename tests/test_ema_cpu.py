"""Parameter EMA on the host side (lidarnerf/nerf/ema.py, LidarTrainer(ema_decay=)): torch_ema's published update rule
restated in the test, the store / copy_to / restore / swap contracts, the "ema" entry of a checkpoint in torch_ema's
state-dict layout, and the argument checks of lnh_ema_update / lnh_ema_swap, which answer without a GPU."""
import ctypes as C
import os

import pytest
import torch


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(257, 2), (16, 32), (7,), (3, 5, 2)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g) * 10.0 ** (i - 2)) for i, s in enumerate(shapes)]
    ps[2].requires_grad_(False)  # averaged all the same (torch_ema is handed model.parameters())
    return ps


def _move(ps, g):
    with torch.no_grad():
        for p in ps:
            p.add_(torch.randn(p.shape, generator=g) * 0.1 * p.abs().mean())


def _model():
    from lidarnerf.nerf.network import NeRFNetwork
    torch.manual_seed(0)
    return NeRFNetwork(encoding="hashgrid", desired_resolution=256, log2_hashmap_size=12, bound=1, min_near=0.01,
                       min_near_lidar=0.01)


@pytest.mark.parametrize("decay, use_num_updates", [(0.95, True), (0.5, True), (0.95, False)])
def test_update_matches_the_written_out_formula(decay, use_num_updates):
    from lidarnerf.nerf.ema import ParameterEMA
    ps = _params()
    ema = ParameterEMA(ps, decay, use_num_updates=use_num_updates)
    assert ema.num_updates == (0 if use_num_updates else None)
    want = [p.detach().clone() for p in ps]
    assert all(torch.equal(s, w) and s.dtype == torch.float32 and s.data_ptr() != p.data_ptr()
               for s, w, p in zip(ema.shadow_params, want, ps))
    g = torch.Generator().manual_seed(1)
    decays = []
    for n in range(1, 26):
        _move(ps, g)
        ema.update()
        d = min(decay, (1 + n) / (10 + n)) if use_num_updates else decay
        decays.append(d)
        one_minus_decay = 1.0 - d
        for s, p in zip(want, ps):
            tmp = s - p.detach()
            tmp.mul_(one_minus_decay)
            s.sub_(tmp)
        assert ema.last_decay == d
        assert ema.num_updates == (n if use_num_updates else None)
        for s, w in zip(ema.shadow_params, want):
            assert torch.equal(s, w), n
    if not use_num_updates:
        assert decays[0] == decay
    elif decay == 0.95:
        assert all(d == (1 + n) / (10 + n) < 0.95 for n, d in enumerate(decays, 1))  # the warm-up rules throughout
        assert (1 + 170) / (10 + 170) == 0.95 and (1 + 169) / (10 + 169) < 0.95
    else:
        assert [d == 0.5 for d in decays] == [n >= 8 for n in range(1, 26)] and decays[0] == 2 / 11
    with pytest.raises(ValueError, match="between 0 and 1"):
        ParameterEMA(ps, 1.5)


def test_store_copy_restore_and_swap_are_exact():
    from lidarnerf.nerf.ema import ParameterEMA
    ps = _params()
    ema = ParameterEMA(ps, 0.5)
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        _move(ps, g)
        ema.update()
    before = [p.detach().clone() for p in ps]
    shadows = [s.clone() for s in ema.shadow_params]
    versions = [p._version for p in ps]
    assert ema.state_dict()["collected_params"] is None
    ema.store()
    assert len(ema.state_dict()["collected_params"]) == len(ps)
    ema.copy_to()
    assert all(torch.equal(p, s) for p, s in zip(ps, shadows)) and not any(torch.equal(p, b) for p, b in zip(ps, before))
    ema.restore()
    assert ema.collected_params is None and all(torch.equal(p, b) for p, b in zip(ps, before))
    with pytest.raises(RuntimeError, match="store"):
        ema.restore()
    ema.swap()
    assert all(torch.equal(p, s) for p, s in zip(ps, shadows))
    assert all(torch.equal(s, b) for s, b in zip(ema.shadow_params, before))
    ema.swap()
    assert all(torch.equal(p, b) for p, b in zip(ps, before))
    assert all(torch.equal(s, w) for s, w in zip(ema.shadow_params, shadows))
    assert [p._version for p in ps] == versions  # (nothing here moves a version counter: captured steps stay valid)
    with pytest.raises(KeyError):
        with ema.average_parameters():
            assert all(torch.equal(p, s) for p, s in zip(ps, shadows))
            raise KeyError("inside")
    assert all(torch.equal(p, b) for p, b in zip(ps, before))
    assert all(torch.equal(s, w) for s, w in zip(ema.shadow_params, shadows))


def test_state_dict_layout_and_load_checks():
    from lidarnerf.nerf.ema import ParameterEMA
    ps = _params()
    ema = ParameterEMA(ps, 0.95)
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        _move(ps, g)
        ema.update()
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert sd["decay"] == 0.95 and sd["num_updates"] == 4 and sd["collected_params"] is None
    assert isinstance(sd["shadow_params"], list) and [tuple(s.shape) for s in sd["shadow_params"]] == [tuple(p.shape) for p in ps]
    other = ParameterEMA(_params(seed=5), 0.5)
    ptrs = [s.data_ptr() for s in other.shadow_params]
    other.load_state_dict(sd)
    assert other.decay == 0.95 and other.num_updates == 4
    assert all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    assert [s.data_ptr() for s in other.shadow_params] == ptrs and ptrs[0] != ema.shadow_params[0].data_ptr()
    with pytest.raises(ValueError, match="3 shadow parameters in the state, 4 parameters here"):
        other.load_state_dict(dict(sd, shadow_params=sd["shadow_params"][:3]))
    bad = list(sd["shadow_params"])
    bad[1] = bad[1].t().contiguous()
    with pytest.raises(ValueError, match=r"shadow parameter 1 has shape \(32, 16\)"):
        other.load_state_dict(dict(sd, shadow_params=bad))


def test_trainer_checkpoint_carries_the_average(tmp_path):
    from lidarnerf.nerf.train_step import LidarTrainer
    keys = {"epoch", "global_step", "stats", "optimizer", "lr_scheduler", "scaler", "model"}
    m = _model()
    tr = LidarTrainer(m, lr=1e-2, fp16=False, ema_decay=0.95)
    assert tr.ema is not None and tr.ema.decay == 0.95 and tr.ema_interval is None
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        _move(list(m.parameters()), g)
        tr.ema_update()
    live = [p.detach().clone() for p in m.parameters()]
    path = tr.save_checkpoint(os.path.join(tmp_path, "ema.pth"))
    ck = torch.load(path, weights_only=False)
    assert set(ck) == keys | {"ema"}
    assert set(ck["ema"]) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert len(ck["ema"]["shadow_params"]) == len(list(m.parameters()))
    assert [tuple(s.shape) for s in ck["ema"]["shadow_params"]] == [tuple(p.shape) for p in m.parameters()]
    assert ck["ema"]["collected_params"] is None and ck["ema"]["num_updates"] == 3 and ck["ema"]["decay"] == 0.95
    assert "ema" not in torch.load(tr.save_checkpoint(os.path.join(tmp_path, "small.pth"), full=False), weights_only=False)
    # round trip into a fresh trainer
    m2 = _model()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)
    tr2 = LidarTrainer(m2, lr=1e-2, fp16=False, ema_decay=0.95)
    tr2.load_checkpoint(path)
    assert tr2.ema.num_updates == 3
    assert all(torch.equal(a, b) for a, b in zip(tr2.ema.shadow_params, tr.ema.shadow_params))
    assert all(torch.equal(a, b) for a, b in zip(m2.parameters(), live))
    # the trainer's own state dict carries it under a key that is absent without an average
    sd = tr.state_dict()
    assert set(sd["ema"]) == set(ck["ema"]) and "ema" not in LidarTrainer(_model(), fp16=False).state_dict()
    tr3 = LidarTrainer(_model(), lr=1e-2, fp16=False, ema_decay=0.95)
    tr3.load_state_dict(sd)
    assert tr3.ema.num_updates == 3 and all(torch.equal(a, b) for a, b in zip(tr3.ema.shadow_params, tr.ema.shadow_params))
    # a trainer WITHOUT an average: today's key set, and it loads a file that carries one
    plain = LidarTrainer(_model(), lr=1e-2, fp16=False)
    assert plain.ema is None
    assert set(torch.load(plain.save_checkpoint(os.path.join(tmp_path, "plain.pth")), weights_only=False)) == keys
    missing, unexpected = plain.load_checkpoint(path)
    assert not missing and not unexpected
    assert all(torch.equal(a, b) for a, b in zip(plain.model.parameters(), live))
    plain.save_checkpoint(os.path.join(tmp_path, "plain.pth"))  # (the loaded parameters, no "ema")
    with pytest.raises(RuntimeError, match="ema_decay"):
        plain.ema_update()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass
    with pytest.raises(ValueError, match="needs ema_decay"):
        LidarTrainer(_model(), fp16=False, ema_interval=2)
    # a trainer WITH an average loading files without one re-seeds: shadow == loaded parameters, num_updates == 0
    for name, kw in (("plain.pth", {}), ("ema.pth", {"model_only": True}), ("bare.pth", {})):
        if name == "bare.pth":
            torch.save(plain.model.state_dict(), os.path.join(tmp_path, name))
        tr4 = LidarTrainer(_model(), lr=1e-2, fp16=False, ema_decay=0.95)
        _move(list(tr4.model.parameters()), g)
        tr4.ema_update()
        tr4.load_checkpoint(os.path.join(tmp_path, name), **kw)
        assert tr4.ema.num_updates == 0, name
        assert all(torch.equal(s, p) for s, p in zip(tr4.ema.shadow_params, tr4.model.parameters())), name
        assert all(torch.equal(p, b) for p, b in zip(tr4.model.parameters(), live)), name
    # ema_model=True: the averaged weights as "model" (the reference's best checkpoint), live parameters untouched
    best = torch.load(tr.save_checkpoint(os.path.join(tmp_path, "best.pth"), full=False, ema_model=True), weights_only=False)
    names = [k for k, _ in m.named_parameters()]
    for k, s, p in zip(names, tr.ema.shadow_params, live):
        assert torch.equal(best["model"][k], s) and not torch.equal(best["model"][k], p), k
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), live))
    assert set(best["model"]) == set(m.state_dict())
    with pytest.raises(RuntimeError, match="ema_decay"):
        plain.save_checkpoint(os.path.join(tmp_path, "no.pth"), ema_model=True)


def test_ema_weights_context_on_the_cpu():
    from lidarnerf.nerf.train_step import LidarTrainer
    m = _model()
    tr = LidarTrainer(m, lr=1e-2, fp16=False, ema_decay=0.5)
    g = torch.Generator().manual_seed(6)
    _move(list(m.parameters()), g)
    tr.ema_update()
    live = [p.detach().clone() for p in m.parameters()]
    shadows = [s.clone() for s in tr.ema.shadow_params]
    with pytest.raises(KeyError):
        with tr.ema_weights() as ema:
            assert ema is tr.ema
            assert all(torch.equal(p, s) for p, s in zip(m.parameters(), shadows))
            raise KeyError("inside")
    assert all(torch.equal(p, b) for p, b in zip(m.parameters(), live))
    assert all(torch.equal(s, w) for s, w in zip(tr.ema.shadow_params, shadows))


def _f32(n, fill=0.0):
    import numpy as np
    buf = np.full(n + 8, fill, dtype=np.float32)
    off = (-buf.ctypes.data % 16) // 4  # a 16-byte aligned window of the buffer
    return buf, buf.ctypes.data + 4 * off


def test_ema_argument_errors_are_reported_without_a_gpu():
    """Validation happens before any launch (tests/test_host_cpu.py checks the other entry points the same way)."""
    from lidarnerf import _hip
    L = _hip.lib()
    (_a, a), (_b, b) = _f32(16), _f32(16)
    vp = lambda *v: C.cast((C.c_void_p * len(v))(*v), C.c_void_p)
    nn = lambda *v: C.cast((C.c_uint32 * len(v))(*v), C.c_void_p)
    many = _hip.TRAIN_MAX_SMALL + 1
    upd = lambda *args: L.lnh_ema_update(*args, None)
    swp = lambda *args: L.lnh_ema_swap(*args, None)
    err = lambda: L.lnh_last_error()
    # nothing to do: fine without a GPU
    assert upd(None, None, 0, None, None, None, 0, 0.05) == 0 and swp(None, None, None, 0, None, None, None, 0) == 0
    assert upd(None, b, 8, None, None, None, 0, 0.05) == -1 and b"ema_update: null table pointer" in err()
    assert upd(a, None, 8, None, None, None, 0, 0.05) == -1 and b"null table pointer" in err()
    assert upd(a + 4, b, 8, None, None, None, 0, 0.05) == -1 and b"16-byte" in err()
    assert upd(a, b + 8, 8, None, None, None, 0, 0.05) == -1 and b"16-byte" in err()
    assert upd(a, a, 8, None, None, None, 0, 0.05) == -1 and b"different buffers" in err()
    assert upd(a, b, 8, vp(*[a] * many), vp(*[b] * many), nn(*[1] * many), many, 0.05) == -1 and b"at most 16 small" in err()
    assert upd(a, b, 8, None, None, None, 1, 0.05) == -1 and b"at most 16 small" in err()
    assert upd(a, b, 8, vp(a + 32), vp(None), nn(4), 1, 0.05) == -1 and b"null small-tensor pointer 0" in err()
    assert upd(a, b, 8, vp(a + 34), vp(b + 32), nn(4), 1, 0.05) == -1 and b"4-byte aligned" in err()
    for w in (-0.5, 1.5, float("nan")):
        assert upd(a, b, 8, None, None, None, 0, w) == -1 and b"one_minus_decay" in err()
    assert swp(None, b, None, 8, None, None, None, 0) == -1 and b"ema_swap: null table pointer" in err()
    assert swp(a, b + 4, None, 8, None, None, None, 0) == -1 and b"16-byte" in err()
    assert swp(a, b, a + 36, 8, None, None, None, 0) == -1 and b"8-byte (fp16)" in err()
    assert swp(a, b, None, 8, vp(*[a] * many), vp(*[b] * many), nn(*[1] * many), many) == -1 and b"at most 16 small" in err()
    assert swp(a, b, None, 8, vp(a + 32), vp(a + 32), nn(4), 1) == -1 and b"different buffers" in err()
    assert _hip._SIGS["lnh_ema_update"][-1] is C.c_float and "lnh_ema_swap" in _hip.EXPORTS


def test_sharded_guards_without_a_process_group():
    """Sharded table optimizer: a rank's fp32 master is current on its own rows only, so averaging it, swapping it or
    copying it is refused until gather_table_state() has completed it; ema_update() and ema_weights() gather first (they
    are collective there) — what of that can be asserted without a process group."""
    from lidarnerf.nerf import fused
    from lidarnerf.nerf.ema import ParameterEMA
    from lidarnerf.nerf.train_step import LidarTrainer
    m = _model()
    tr = LidarTrainer(m, lr=1e-2, fp16=False, ema_decay=0.95)
    emb = m.encoder.embeddings
    assert any(p is emb for p in tr.ema._params)
    shadows = [s.clone() for s in tr.ema.shadow_params]
    emb._lnh_master_stale = True
    for call in (tr.ema.update, tr.ema.swap, tr.ema.store, tr.ema.copy_to, tr.ema.reseed):
        with pytest.raises(RuntimeError, match="gather_table_state"):
            call()
    assert tr.ema.num_updates == 0 and all(torch.equal(a, b) for a, b in zip(tr.ema.shadow_params, shadows))
    # the trainer's calls gather first: with the table marked sharded they reach for the process group
    calls = []
    tr.table, tr.sharded = emb, True
    tr.gather_table_state = lambda: (calls.append(1), setattr(emb, "_lnh_master_stale", False))[0]
    tr.ema_update()
    assert calls == [1] and tr.ema.num_updates == 1
    emb._lnh_master_stale = True
    with tr.ema_weights():
        assert calls == [1, 1] and emb._lnh_ema_weights is True
    assert not hasattr(emb, "_lnh_ema_weights")
    for doc in (LidarTrainer.ema_update.__doc__, LidarTrainer.ema_weights.__doc__):
        assert "COLLECTIVE" in doc and "gather_table_state" in doc
    # table16_of: the early return exists under the trainer's mark only, and only for evaluation
    tr.table, tr.sharded = None, False
    emb._lnh_table16 = emb.detach().half().reshape(-1, 2).contiguous()
    emb._lnh_table16_version = emb._version
    assert fused.table16_of(emb, training=False) is not emb._lnh_table16
    emb._lnh_ema_weights = True
    assert fused.table16_of(emb, training=False) is emb._lnh_table16
    del emb._lnh_ema_weights
    assert fused.table16_of(emb, training=False).data_ptr() != emb._lnh_table16.data_ptr()
    assert isinstance(tr.ema, ParameterEMA)
