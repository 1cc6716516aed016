"""The ray-drop MLP kernels and trainer on the device (csrc/raydrop.hip, lidarnerf/raydrop.py).

1. Exact known answers through the C ABI on the integer-valued problems of tests/raydrop_ref.py (tests/test_raydrop_cpu.py asserts
   what makes them exact): outputs, the loss (ONE division of the exact numerator) and every gradient (ONE division of the exact
   sum; for the L1 loss the sums are sums of the signs) compared with torch.equal, never within a bound.  Sizes 1, 15, 16, 17, 63,
   64, 65, 127, 128, 129, 257 sit on either side of the row tile chosen (16) and of the weight-gradient kernel's wave chunks and
   32-row trips (raydrop_ref.py).
   Outputs are sentinel-filled with 64 guard words, inputs carry 64 NaN rows behind row N, the workspace is NaN-filled, grad is
   pre-filled (it is overwritten), and every call is made twice and must be bit-identical.
2. G16 (the reference's module in float64): outputs, loss and each gradient tensor within 4 x the reference's own fp32 deviation,
   never less than one fp32 ulp of the tensor's largest magnitude.
3. Adam: 1 and 20 steps on G16's batches by max |dp| / lr under the same rule; the lr_table lookup and the step counter over 30
   steps, past the end of the table.
4. Stride and hipGraph capture.  5. The trainer: epoch boundary, determinism, checkpoints.  6. Learning against G16's record.
"""
import functools
import os

import numpy as np
import pytest
import torch

import raydrop_ref as rr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD, POISON_ROWS, SENT = 64, 64, -3.0e6  # (no expected value of an exact case reaches the sentinel: all are below 2^24 / B)


@functools.lru_cache(maxsize=None)
def _g16(name="g16_raydrop"):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """n floats of `fill`, then GUARD sentinel words."""

    def __init__(self, n, fill=SENT):
        self.n = n
        self.buf = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
        self.buf[:n] = fill

    def data(self):
        return self.buf[:self.n]

    def ptr(self):
        return self.buf.data_ptr()

    def check(self, want, what):
        assert bool((self.buf[self.n:] == SENT).all()), f"{what}: guard words behind the buffer were overwritten"
        got = self.data()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements differ, first at {bad[0].item()}: "
                                 f"got {got[bad[0]].item()}, want {want[bad[0]].item()}")


def _poisoned(rows):
    """The rows with POISON_ROWS rows of NaN behind them."""
    flat = torch.full(((rows.shape[0] + POISON_ROWS) * rows.shape[1],), float("nan"), dtype=torch.float32, device="cuda")
    flat[:rows.numel()] = rows.reshape(-1)
    return flat


def _forward(params, D, W, rows, stride, N, out_ptr):
    from lidarnerf import _hip
    _hip.call("lnh_raydrop_forward", params.data_ptr(), D, W, rows.data_ptr(), stride, N, out_ptr)


def _workspace(D, W, B):
    """NaN-filled workspace of exactly the size asked for, then GUARD words of NaN with a known bit pattern."""
    from lidarnerf import _hip
    need = int(_hip.lib().lnh_raydrop_workspace_size(D, W, B))
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return ws, need


def _grad(params, D, W, rows, B, loss_type, ws, need, loss_ptr, grad_ptr):
    from lidarnerf import _hip
    _hip.call("lnh_raydrop_grad", params.data_ptr(), D, W, rows.data_ptr(), B, loss_type, ws.data_ptr(), need, loss_ptr, grad_ptr)


def _adam(p, m, v, g, table, steps, cur):
    from lidarnerf import _hip
    _hip.call("lnh_raydrop_adam", p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), p.numel(), table.data_ptr(),
              table.numel(), steps.data_ptr() + 4 * cur, steps.data_ptr() + 4 * (1 - cur), 0.9, 0.999, 1e-8)
    return 1 - cur


# ------------------------------------------------------------------------------------------------ 1. exact known answers
@functools.lru_cache(maxsize=None)
def _exact(D, W, B, loss_type):
    params, rows = rr.exact_case(D, W, B, loss_type)
    parts = {}
    out, num, _loss, _grad64 = rr.loss_and_grad(params, D, W, rows, loss_type, parts)
    want_loss = np.float32(num) / np.float32(B)
    want_grad = parts["gsum"].astype(np.float32) / np.float32(B)
    assert np.array_equal(parts["gsum"].astype(np.float32).astype(np.float64), parts["gsum"])
    return _dev(params), _dev(rows), _dev(out), torch.tensor([want_loss], device="cuda"), _dev(want_grad)


@pytest.mark.parametrize("D,W", rr.EXACT_SHAPES)
def test_forward_exact(D, W):
    for N in rr.EXACT_SIZES:
        params, rows, want, _, _ = _exact(D, W, N, 0)
        for cols in (6, 5):
            src = _poisoned(rows[:, :cols].contiguous())
            outs = []
            for _ in range(2):
                o = Out(N)
                _forward(params, D, W, src, cols, N, o.ptr())
                o.check(want, f"forward D={D} W={W} N={N} stride={cols}")
                outs.append(o)
            assert torch.equal(_bits(outs[0].buf), _bits(outs[1].buf))


@pytest.mark.parametrize("loss_type", [0, 1])
@pytest.mark.parametrize("D,W", rr.EXACT_SHAPES)
def test_grad_exact(D, W, loss_type):
    for B in rr.EXACT_SIZES:
        params, rows, _, want_loss, want_grad = _exact(D, W, B, loss_type)
        src = _poisoned(rows)
        runs = []
        for fill in (SENT, 2.0):  # grad is overwritten, not added to: whatever it held
            ws, need = _workspace(D, W, B)
            loss, grad = Out(1), Out(params.numel(), fill)
            _grad(params, D, W, src, B, loss_type, ws, need, loss.ptr(), grad.ptr())
            what = f"D={D} W={W} B={B} loss_type={loss_type}"
            loss.check(want_loss, "loss " + what)
            grad.check(want_grad, "grad " + what)
            assert bool(torch.isnan(ws[need // 4:]).all()), "workspace: written past the size asked for"
            runs.append((loss, grad))
        assert torch.equal(_bits(runs[0][0].data()), _bits(runs[1][0].data()))
        assert torch.equal(_bits(runs[0][1].data()), _bits(runs[1][1].data()))
        assert torch.equal(_bits(src[:rows.numel()]), _bits(rows.reshape(-1)))  # the inputs are read only


# ---------------------------------------------------------------------------------------------------------------- 2. G16
def _tolerance(dev, magnitude):
    return max(4.0 * float(dev), float(np.spacing(np.float32(magnitude))))


def _tensors(flat, D, W):
    out = []
    for w, b in rr.split(flat, D, W):
        out += [w.reshape(-1), b]
    return out


def test_g16_forward_loss_and_gradients():
    g, gl1 = _g16(), _g16("g16_raydrop_l1")
    D, W = 4, 128
    params, rows = _dev(g["params"]), _dev(g["rows"])
    out = torch.empty(256, device="cuda")
    _forward(params, D, W, rows, 6, 256, out.data_ptr())
    dev = np.abs(out.cpu().numpy().astype(np.float64) - g["out64"]).max()
    tol = _tolerance(g["dev_out"], np.abs(g["out64"]).max())
    print(f"out: device deviates by {dev:.3g}, the reference's fp32 by {float(g['dev_out']):.3g}, allowed {tol:.3g}")
    assert dev <= tol
    for name, lt, want in (("mse", 0, g["grad64_mse"]), ("l1", 1, gl1["grad64_l1"])):
        ws, need = _workspace(D, W, 256)
        loss, grad = torch.empty(1, device="cuda"), torch.empty(params.numel(), device="cuda")
        _grad(params, D, W, rows, 256, lt, ws, need, loss.data_ptr(), grad.data_ptr())
        l64 = float(g[f"loss64_{name}"])
        dev, tol = abs(float(loss.item()) - l64), _tolerance(g[f"dev_loss_{name}"], abs(l64))
        print(f"loss {name}: device deviates by {dev:.3g}, the reference's fp32 by {float(g[f'dev_loss_{name}']):.3g}, allowed {tol:.3g}")
        assert dev <= tol
        got = _tensors(grad.cpu().numpy().astype(np.float64), D, W)
        failed = []
        for k, (a, b) in enumerate(zip(got, _tensors(want, D, W))):
            dev, tol = np.abs(a - b).max(), _tolerance(g[f"dev_grad_{name}"][k], np.abs(b).max())
            print(f"grad {name} tensor {k}: device deviates by {dev:.3g}, the reference's fp32 by {g[f'dev_grad_{name}'][k]:.3g}, "
                  f"allowed {tol:.3g}")
            if dev > tol:
                failed.append(k)
        assert not failed, failed


# --------------------------------------------------------------------------------------------------------------- 3. Adam
def test_adam_one_and_twenty_steps_against_float64():
    g, ga = _g16(), _g16("g16_raydrop_adam")
    D, W, lr = 4, 128, 5e-4
    batches = _dev(ga["batches"])
    table = _dev(g["lr_exp"])
    p = _dev(g["params"])
    P = p.numel()
    m, v, grad = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda"), torch.empty(P, device="cuda")
    loss, steps, cur = torch.empty(1, device="cuda"), torch.zeros(2, device="cuda"), 0
    ws, need = _workspace(D, W, 64)
    for k in range(20):
        _grad(p, D, W, batches[k], 64, 0, ws, need, loss.data_ptr(), grad.data_ptr())
        cur = _adam(p, m, v, grad, table, steps, cur)
        if k in (0, 19):
            want = ga[f"p64_{k + 1}"]
            dev = np.abs(p.cpu().numpy().astype(np.float64) - want).max() / lr
            tol = max(4.0 * float(ga[f"dev_p_{k + 1}"]), float(np.spacing(np.float32(np.abs(want).max()))) / lr)
            print(f"Adam, {k + 1} steps: device deviates by {dev:.3g} lr, the reference's fp32 by {float(ga[f'dev_p_{k + 1}']):.3g} lr, "
                  f"allowed {tol:.3g} lr")
            assert dev <= tol
    assert steps.tolist()[cur] == 20.0


def test_adam_table_lookup_and_step_counter():
    """A constant gradient of 1 makes Adam's bias-corrected ratio 1 / (1 + eps) at every step, so step k moves every parameter by
    lr_table[min(k, len - 1)] (to the rounding of the running sum: ulp(0.2) = 1.5e-8 against rates of 1e-3 and more)."""
    n, lr_len = 1000, 7
    table = torch.tensor([1e-3 * (k + 1) for k in range(lr_len)], device="cuda")
    p, m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    g, steps, cur = torch.ones(n, device="cuda"), torch.zeros(2, device="cuda"), 0
    before = p.clone()
    for k in range(30):
        cur = _adam(p, m, v, g, table, steps, cur)
        moved = before - p
        want = 1e-3 * (min(k, lr_len - 1) + 1)
        assert float(moved.min()) == float(moved.max()) and abs(float(moved[0]) - want) <= 1e-4 * want, (k, float(moved[0]), want)
        assert steps.tolist()[cur] == k + 1.0
        before = p.clone()


# ------------------------------------------------------------------------------------------------- 4. stride and capture
def test_forward_ignores_the_columns_behind_the_fifth():
    g = _g16()
    params, rows = _dev(g["params"]), _dev(g["learn_rows"][:1001])
    a, b = torch.empty(1001, device="cuda"), torch.empty(1001, device="cuda")
    _forward(params, 4, 128, rows, 6, 1001, a.data_ptr())
    _forward(params, 4, 128, rows[:, :5].contiguous(), 5, 1001, b.data_ptr())
    assert torch.equal(_bits(a), _bits(b)) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


def test_captured_graph_replays_equal_eager_steps():
    """grad + adam twice (the step counter is double-buffered: two steps bring it back to its first slot) captured in a hipGraph
    and replayed five times, against ten eager steps: parameters, moments, loss and the counter bit for bit."""
    g = _g16()
    D, W, B = 4, 128, 200
    batch = _dev(g["learn_rows"][:B])
    table = _dev(g["lr_exp"])

    def state():
        p = _dev(g["params"])
        return [p, torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p), torch.empty(1, device="cuda"),
                torch.zeros(2, device="cuda")]

    def two_steps(s, ws, need):
        p, m, v, grad, loss, steps = s
        cur = 0
        for _ in range(2):
            _grad(p, D, W, batch, B, 0, ws, need, loss.data_ptr(), grad.data_ptr())
            cur = _adam(p, m, v, grad, table, steps, cur)

    ws, need = _workspace(D, W, B)
    eager = state()
    for _ in range(5):
        two_steps(eager, ws, need)
    torch.cuda.synchronize()
    replayed = state()
    graph = torch.cuda.CUDAGraph()
    backup = [t.clone() for t in replayed]
    with torch.cuda.graph(graph):
        two_steps(replayed, ws, need)
    for t, b in zip(replayed, backup):  # (capture runs nothing; be sure of the starting point all the same)
        t.copy_(b)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(_bits(a), _bits(b)), k
    assert eager[5].tolist() == [10.0, 9.0]


# ------------------------------------------------------------------------------------------------------------ 5. trainer
def _table(M, seed=2):
    g = _g16()
    rng = np.random.default_rng(seed)
    return _dev(g["learn_rows"][rng.permutation(8192)[:M]])


def _model(D=2, W=128, seed=1):
    from lidarnerf.raydrop import RayDropMLP
    torch.manual_seed(seed)
    return RayDropMLP(D, W).cuda()


def test_trainer_epoch_boundary():
    """M = 5 N_rand + 7: five full batches, a short one of 7 rows, the reshuffle and the cursor — against the same steps made by
    hand through the C ABI on slices of the table."""
    from lidarnerf.raydrop import RayDropTrainer
    N_rand, D, W = 64, 2, 128
    M = 5 * N_rand + 7
    rows = _table(M)
    model = _model(D, W)
    tr = RayDropTrainer(model, rows, N_rand=N_rand, N_iters=100, seed=9)
    p = model.flat.clone()
    m, v, grad = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    loss, steps, cur = torch.empty(1, device="cuda"), torch.zeros(2, device="cuda"), 0
    ws, need = _workspace(D, W, N_rand)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    mine, cursor = rows.clone(), 0
    for k in range(14):
        batch = mine[cursor:cursor + N_rand]
        assert batch.shape[0] == (7 if k % 6 == 5 else N_rand) and tr.cursor == cursor
        _grad(p, D, W, batch, batch.shape[0], 0, ws, need, loss.data_ptr(), grad.data_ptr())
        cur = _adam(p, m, v, grad, tr.lr_table, steps, cur)
        cursor += N_rand
        if cursor >= M:
            mine = mine[torch.randperm(M, device="cuda", generator=gen)]
            cursor = 0
        got = tr.step()
        assert torch.equal(_bits(got), _bits(loss)) and torch.equal(_bits(model.flat), _bits(p)), k
        assert torch.equal(_bits(tr.rows), _bits(mine)) and tr.global_step == k + 1
    assert tr.cursor == 2 * N_rand and tr.adam_step == 14
    # the table was reshuffled twice and is still the same set of rows
    assert not torch.equal(tr.rows, rows)
    assert np.array_equal(np.unique(rows.cpu().numpy(), axis=0), np.unique(tr.rows.cpu().numpy(), axis=0))
    assert bool(torch.isfinite(model.flat).all())


def test_two_trainers_of_one_seed_are_bit_identical():
    from lidarnerf.raydrop import RayDropTrainer
    rows = _table(700)
    runs = []
    for _ in range(2):
        model = _model()
        tr = RayDropTrainer(model, rows.clone(), N_rand=128, N_iters=100, seed=4, cosLR=True, warmup_iters=5, loss="l1loss")
        losses = torch.stack([tr.step().clone() for _ in range(30)])
        runs.append((model.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), losses))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(torch.isfinite(runs[0][3]).all())


def test_checkpoint_continues_bit_identically(tmp_path):
    from lidarnerf.raydrop import RayDropTrainer
    rows = _table(700)
    model = _model()
    tr = RayDropTrainer(model, rows, N_rand=128, N_iters=100, seed=4)
    for _ in range(10):  # (one epoch boundary at step 6)
        tr.step()
    path = str(tmp_path / "000010.tar")
    tr.save_checkpoint(path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert {"global_step", "network_fn_state_dict", "optimizer_state_dict"} <= set(ckpt) and ckpt["global_step"] == 10
    other = _model(seed=77)
    assert not torch.equal(other.flat, model.flat)
    tr2 = RayDropTrainer(other, tr.rows.clone(), N_rand=128, N_iters=100, seed=123)
    tr2.load_checkpoint(path)
    assert tr2.global_step == 10 and tr2.adam_step == 10 and tr2.cursor == tr.cursor
    for t in (tr, tr2):
        t.losses = torch.stack([t.step().clone() for _ in range(15)])  # (two more epoch boundaries)
    assert torch.equal(_bits(tr.losses), _bits(tr2.losses)) and torch.equal(_bits(model.flat), _bits(other.flat))
    assert torch.equal(_bits(tr.exp_avg_sq), _bits(tr2.exp_avg_sq)) and torch.equal(_bits(tr.rows), _bits(tr2.rows))
    # a stock torch.optim.Adam over stock modules of the same names loads the checkpoint
    stock = torch.nn.Module()
    stock.linears = torch.nn.ModuleList([torch.nn.Linear(5, 128), torch.nn.Linear(128, 128)])
    stock.output_linear = torch.nn.Linear(128, 1)
    stock.load_state_dict(ckpt["network_fn_state_dict"])
    opt = torch.optim.Adam(stock.parameters(), lr=1.0)
    opt.load_state_dict(ckpt["optimizer_state_dict"])
    assert float(opt.state[stock.output_linear.bias]["step"]) == 10


# ----------------------------------------------------------------------------------------------------------- 6. learning
def test_learning_lands_where_the_reference_loop_lands():
    """G16's record of five shuffles of the reference's own loop (300 steps, N_rand 256, default exponential schedule):
    mean training loss of the last 50 steps 0.0499, 0.0478, 0.0478, 0.0496, 0.0553; held-out accuracy 0.9531, 0.9600, 0.9648,
    0.9790, 0.9463.  The device trainer must land within one range-width outside that range."""
    from lidarnerf.raydrop import RayDropMLP, RayDropTrainer
    g = _g16()
    lo, hi = float(g["learn_loss"].min()), float(g["learn_loss"].max())
    lo_acc, hi_acc = float(g["learn_acc"].min()), float(g["learn_acc"].max())
    torch.manual_seed(0)
    model = RayDropMLP(4, 128).cuda()
    rows = _dev(g["learn_rows"])
    rows = rows[torch.randperm(8192, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))]
    tr = RayDropTrainer(model, rows, N_rand=256, seed=0)
    losses = torch.stack([tr.step().clone() for _ in range(300)]).reshape(-1)
    loss = float(losses[-50:].mean())
    held = _dev(g["learn_heldout"])
    acc = float(((model(held).reshape(-1) > 0.5) == (held[:, 5] > 0.5)).float().mean())
    assert torch.equal(model.predict_mask(held), (model(held) > 0.5).float())
    print(f"device trainer: mean loss of the last 50 steps {loss:.5f} (reference {lo:.5f} .. {hi:.5f}), held-out accuracy "
          f"{acc:.4f} (reference {lo_acc:.4f} .. {hi_acc:.4f})")
    assert loss <= hi + (hi - lo) and acc >= lo_acc - (hi_acc - lo_acc)
