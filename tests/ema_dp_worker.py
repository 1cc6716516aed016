"""Worker of tests/test_ema_gpu.py (not a test module): run under torch.distributed.run with 2 ranks (gloo, both on GPU 0).
The parameter average with the SHARDED table optimizer — a rank's fp32 master is current on its own rows only, so
ema_update() and entering ema_weights() gather first — against the same step with the replicated optimizer in the same
2-rank world: one sharded step is bit-identical to the replicated one (tests/dp_worker.py), so everything here is too."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "lidar-nerf_amd"))
os.environ.setdefault("LNH_DIST_BACKEND", "gloo")
import torch, bench
from lidarnerf import parallel
from lidarnerf.nerf.train_step import LidarTrainer
rank, local, world = parallel.init_from_env()
assert world == 2, world
torch.cuda.set_device(0)
device = torch.device("cuda", 0)
poses = bench.synthetic_frames(60, device)
bits = lambda t: t.detach().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)
same = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def run(sharded):
    torch.manual_seed(0)
    m = bench.build_model(device)
    parallel.broadcast_parameters(m)
    t = LidarTrainer(m, fp16=True, scale=bench.SCALE, world_size=world, render_kwargs=dict(num_steps=768, upsample_steps=64),
                     shard_table_optimizer=sharded, ema_decay=0.95)
    assert t.sharded == sharded and t.ema is not None
    tp = t.table
    init = [p.detach().clone() for p in m.parameters()]
    torch.manual_seed(100)
    t.step(*bench.make_batch(poses, 0, 512, rank, device))   # different rays on every rank
    assert tp._lnh_master_stale == sharded
    if sharded:
        try:
            t.ema.update()   # the bare average refuses a master that is current on this rank's rows only
            raise SystemExit("ParameterEMA.update on a stale sharded master did not raise")
        except RuntimeError as e:
            assert "gather_table_state" in str(e) and t.ema.num_updates == 0
    t.ema_update()           # collective when sharded
    assert not tp._lnh_master_stale and t.ema.num_updates == 1
    state = {"shadows": [s.clone() for s in t.ema.shadow_params], "master": tp.detach().clone(),
             "table16": tp._lnh_table16.clone(), "live": [p.detach().clone() for p in m.parameters()]}
    # the formula on this rank's own tensors: decay = min(0.95, 2 / 11)
    for s, p0, p in zip(state["shadows"], init, state["live"]):
        want = p0.clone()
        tmp = want - p
        tmp.mul_(1.0 - 2 / 11)
        want.sub_(tmp)
        assert same(s, want)
    with t.ema_weights():
        assert all(same(p, s) for p, s in zip(m.parameters(), state["shadows"]))
        assert same(tp._lnh_table16, tp.detach().half().reshape(-1, 2)) and not same(tp._lnh_table16, state["table16"])
        assert not tp._lnh_master_stale
    state["after"] = (tp.detach().clone(), tp._lnh_table16.clone(), bool(tp._lnh_master_stale),
                      [s.clone() for s in t.ema.shadow_params])
    return state


a, b = run(False), run(True)
for name in ("master", "table16"):
    assert same(a[name], b[name]), f"rank {rank}: sharded differs from replicated in {name}"
for i, (x, y) in enumerate(zip(a["shadows"], b["shadows"])):
    assert same(x, y), f"rank {rank}: shadow {i} of the sharded run differs from the replicated one"
for st in (a, b):
    master, t16, stale, shadows = st["after"]
    assert same(master, st["master"]) and same(t16, st["table16"]) and stale is False
    assert all(same(x, y) for x, y in zip(shadows, st["shadows"]))
assert same(a["after"][0], b["after"][0]) and same(a["after"][1], b["after"][1])
# every rank formed the same average without talking about it
chk = torch.stack([s.double().sum() for s in b["shadows"]])
all_chk = [torch.zeros_like(chk) for _ in range(world)]
torch.distributed.all_gather(all_chk, chk)
assert all(torch.equal(c, all_chk[0]) for c in all_chk)
print(f"rank {rank}: EMA-DP-OK", flush=True)
if torch.distributed.is_initialized():
    torch.cuda.synchronize()
    torch.distributed.destroy_process_group()
