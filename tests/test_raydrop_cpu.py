"""Host side of the ray-drop MLP (csrc/raydrop.hip, lidarnerf/raydrop.py): exports and signatures, every argument refusal, the
parameter count, state-dict names, the checkpoint layout against stock torch modules, the learning-rate table against the
reference's sequences (G16), the NumPy restatement (tests/raydrop_ref.py) against G16's float64 tensors, and the conditions that
make the exact known-answer tests of tests/test_raydrop_gpu.py meaningful."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import raydrop_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID_ARG = -1  # LNH_ERR_INVALID_ARG (include/lidarnerf_hip.h)
NAMES = ("lnh_raydrop_forward", "lnh_raydrop_grad", "lnh_raydrop_adam")


def _g16(name="g16_raydrop"):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_exports_and_signatures():
    from lidarnerf import _hip
    L = _hip.lib()
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    for name in NAMES + ("lnh_raydrop_workspace_size", "lnh_raydrop_param_count"):
        assert name in _hip.EXPORTS and hasattr(L, name) and name in text, name
    for name in NAMES:
        assert name in _hip._SIGS
    assert len(_hip._SIGS["lnh_raydrop_forward"]) == 7 and len(_hip._SIGS["lnh_raydrop_grad"]) == 10
    assert len(_hip._SIGS["lnh_raydrop_adam"]) == 12 and _hip._SIGS["lnh_raydrop_adam"][-3:] == [C.c_double] * 3


def test_parameter_count_and_workspace_size():
    from lidarnerf import _hip, raydrop
    L = _hip.lib()
    assert L.lnh_raydrop_param_count(4, 128) == raydrop.param_count(4, 128) == rr.param_count(4, 128) == 50433
    for D in range(1, 9):
        for W in (128, 256):
            assert L.lnh_raydrop_param_count(D, W) == raydrop.param_count(D, W) == W * 5 + W + (D - 1) * (W * W + W) + W + 1
            for B in (1, 16, 17, 2048):
                bpad = (B + 15) // 16 * 16
                assert L.lnh_raydrop_workspace_size(D, W, B) == 4 * (2 * D * W * bpad + bpad + bpad // 16)
    for D, W, B in ((0, 128, 16), (9, 128, 16), (4, 64, 16), (4, 192, 16), (4, 512, 16), (4, 128, 0)):
        assert L.lnh_raydrop_workspace_size(D, W, B) == 0
    assert L.lnh_raydrop_param_count(4, 64) == 0 and L.lnh_raydrop_param_count(0, 128) == 0


def test_every_argument_refusal():
    """Validation happens before any launch, so it runs without a GPU (the pointers are never dereferenced)."""
    from lidarnerf import _hip
    L = _hip.lib()
    p = 1 << 20  # a 16-byte aligned non-null "pointer"

    def err():
        return L.lnh_last_error().decode()

    assert L.lnh_raydrop_forward(p, 4, 128, p, 5, 0, p, None) == 0  # no rows: nothing to do
    for D, W in ((4, 64), (0, 128), (9, 128), (4, 192), (4, 0)):
        assert L.lnh_raydrop_forward(p, D, W, p, 5, 16, p, None) == INVALID_ARG and "W must be 128 or 256" in err()
        assert L.lnh_raydrop_grad(p, D, W, p, 16, 0, p, 1 << 30, p, p, None) == INVALID_ARG and "W must be 128 or 256" in err()
    assert L.lnh_raydrop_forward(p, 4, 128, p, 4, 16, p, None) == INVALID_ARG and "at least 5 columns" in err()
    assert L.lnh_raydrop_forward(None, 4, 128, p, 5, 16, p, None) == INVALID_ARG and "null" in err()
    assert L.lnh_raydrop_forward(p, 4, 128, None, 5, 16, p, None) == INVALID_ARG
    assert L.lnh_raydrop_forward(p, 4, 128, p, 5, 16, None, None) == INVALID_ARG
    assert L.lnh_raydrop_forward(p + 4, 4, 128, p, 5, 16, p, None) == INVALID_ARG and "aligned" in err()
    need = L.lnh_raydrop_workspace_size(4, 128, 100)
    assert need > 0
    assert L.lnh_raydrop_grad(p, 4, 128, p, 100, 0, None, need, p, p, None) == INVALID_ARG and "null" in err()
    assert L.lnh_raydrop_grad(p, 4, 128, p, 100, 0, p, need - 1, p, p, None) == INVALID_ARG and "workspace" in err()
    assert L.lnh_raydrop_grad(p, 4, 128, p, 100, 0, p, 0, p, p, None) == INVALID_ARG
    assert L.lnh_raydrop_grad(p, 4, 128, p, 0, 0, p, need, p, p, None) == INVALID_ARG and "batch" in err()
    assert L.lnh_raydrop_grad(p, 4, 128, p, 100, 2, p, need, p, p, None) == INVALID_ARG and "loss_type" in err()
    assert L.lnh_raydrop_grad(p, 4, 128, p, 100, 0, p + 8, need, p, p, None) == INVALID_ARG and "aligned" in err()
    for k in (0, 3, 7, 8):  # loss, grad, params, rows
        args = [p, 4, 128, p, 100, 0, p, need, p, p]
        args[{0: 8, 3: 9, 7: 0, 8: 3}[k]] = None
        assert L.lnh_raydrop_grad(*args, None) == INVALID_ARG and "null" in err()
    b = (C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8))
    assert L.lnh_raydrop_adam(p, p, p, p, 10, p, 4, p, p, *b, None) == INVALID_ARG and "double-buffered" in err()
    assert L.lnh_raydrop_adam(p, p, p, p, 10, p, 0, p, p + 4, *b, None) == INVALID_ARG and "table" in err()
    for k in (0, 1, 2, 3, 5, 7, 8):
        args = [p, p, p, p, 10, p, 4, p, p + 4]
        args[k] = None
        assert L.lnh_raydrop_adam(*args, *b, None) == INVALID_ARG and "null" in err()


def test_python_layer_refusals():
    from lidarnerf.raydrop import RayDropMLP, lr_table
    for D, W in ((4, 64), (0, 128), (9, 256)):
        with pytest.raises(ValueError, match="W must be 128 or 256"):
            RayDropMLP(D, W)
    with pytest.raises(NotImplementedError, match="identity embedding"):
        RayDropMLP(4, 128, i_embed=0)
    m = RayDropMLP(2, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_mask(torch.zeros(4, 5))
    with pytest.raises(ValueError, match="do not outlast"):
        lr_table(10, cosLR=True, warmup_iters=10)


def test_state_dict_names_shapes_and_the_flat_buffer():
    from lidarnerf.raydrop import RayDropMLP
    torch.manual_seed(3)
    m = RayDropMLP(4, 128)
    sd = m.state_dict()
    want = [("linears.0.weight", (128, 5)), ("linears.0.bias", (128,))]
    for l in range(1, 4):
        want += [(f"linears.{l}.weight", (128, 128)), (f"linears.{l}.bias", (128,))]
    want += [("output_linear.weight", (1, 128)), ("output_linear.bias", (1,))]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert m.flat.shape == (50433,) and m.flat.dtype == torch.float32
    # the parameters ARE the flat buffer, in order
    assert torch.equal(torch.cat([p.reshape(-1) for p in m.parameters()]), m.flat)
    o = 0
    for p in m.parameters():
        assert p.data_ptr() == m.flat.data_ptr() + 4 * o
        o += p.numel()
    # the reference's initialisation: kaiming-normal weights (std sqrt(2 / fan_in)), zero biases
    assert all(float(lin.bias.abs().max()) == 0 for lin in list(m.linears) + [m.output_linear])
    assert abs(float(m.linears[1].weight.std()) - (2 / 128) ** 0.5) < 0.01 * (2 / 128) ** 0.5 * 3
    assert abs(float(m.linears[0].weight.std()) - (2 / 5) ** 0.5) < 0.15 * (2 / 5) ** 0.5
    # load_state_dict of a stock module chain of the reference's names writes THROUGH to the flat buffer
    ref = _stock(4, 128)
    m.load_state_dict(ref.state_dict())
    assert torch.equal(m.flat, torch.cat([p.detach().reshape(-1) for p in ref.parameters()]))
    big = RayDropMLP(8, 256)
    assert big.num_parameters == rr.param_count(8, 256) == len(big.flat)


class _Stock(torch.nn.Module):
    """The reference's module structure from stock layers (names linears.{l}, output_linear)."""

    def __init__(self, D, W):
        super().__init__()
        self.linears = torch.nn.ModuleList([torch.nn.Linear(5, W)] + [torch.nn.Linear(W, W) for _ in range(D - 1)])
        self.output_linear = torch.nn.Linear(W, 1)


def _stock(D, W):
    return _Stock(D, W)


def test_learning_rate_tables_equal_the_references_sequences():
    from lidarnerf.raydrop import lr_table
    g = _g16()
    exp = lr_table(500000)
    cos = lr_table(500000, cosLR=True)
    short = lr_table(40, cosLR=True, warmup_iters=10)
    assert len(exp) == len(cos) == 500000 and len(short) == 40
    for got, want in ((exp, g["lr_exp"]), (cos, g["lr_cos"]), (short, g["lr_cos_short"])):
        assert np.array_equal(got[:30].astype(np.float32), want.astype(np.float32))
    # the one-step lag: the first TWO steps of the exponential schedule run at lrate, the cosine warm-up starts from 0 at step 1
    assert exp[0] == exp[1] == 5e-4 and exp[2] < 5e-4 and cos[0] == 5e-4 and cos[1] == 0.0 and short[11] == 5e-4
    assert np.all(np.diff(short[11:]) < 0)


def test_restatement_equals_g16_float64():
    g, gl1 = _g16(), _g16("g16_raydrop_l1")
    params, rows = g["params"].astype(np.float64), g["rows"].astype(np.float64)
    assert g["params"].dtype == np.float32 and len(params) == 50433 and rows.shape == (256, 6)
    assert (rows[:, 3] == 0).sum() == 256 // 5 and np.allclose(np.linalg.norm(rows[:, :3], axis=1), 1, atol=1e-6)
    for name, lt, want in (("mse", 0, g["grad64_mse"]), ("l1", 1, gl1["grad64_l1"])):
        out, num, loss, grad = rr.loss_and_grad(params, 4, 128, rows, lt)
        assert np.abs(out - g["out64"]).max() <= 1e-12 * np.abs(g["out64"]).max()
        assert abs(loss - float(g[f"loss64_{name}"])) <= 1e-12 * abs(loss)
        assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()
    # Adam: the restated step on the restated gradients walks to the stored float64 parameters
    ga = _g16("g16_raydrop_adam")
    p, m, v = params.copy(), np.zeros_like(params), np.zeros_like(params)
    for k in range(20):
        grad = rr.loss_and_grad(p, 4, 128, ga["batches"][k].astype(np.float64), 0)[3]
        p, m, v = rr.adam(p, m, v, grad, k, g["lr_exp"][k])
        if k == 0:
            assert np.abs(p - ga["p64_1"]).max() <= 1e-12 * np.abs(p).max()
    assert np.abs(p - ga["p64_20"]).max() <= 1e-9 * np.abs(p).max()  # (twenty steps amplify the last bit of a tiny gradient)


def test_fixture_sizes():
    for name in ("g16_raydrop", "g16_raydrop_l1", "g16_raydrop_adam"):
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < (1 << 20)
    g = _g16()
    assert g["learn_rows"].shape == (8192, 6) and g["learn_heldout"].shape == (2048, 6) and len(g["learn_loss"]) == 5
    t = g["learn_rows"]
    assert np.array_equal(t[:, 5], ((t[:, 3] > 0) & (t[:, 2] < 0.2)).astype(np.float32))


@pytest.mark.parametrize("D,W", rr.EXACT_SHAPES)
def test_exact_cases_are_exact_and_exercise_what_they_claim(D, W):
    """In exact integer arithmetic every sum of absolute products of every exact case stays below 2^24 (so every partial sum in
    every order is representable), every value is an integer, and the cases reach every layer: a non-zero weight and bias
    gradient per layer, both ReLU branches per layer, both signs and the zero of the L1 gradient."""
    for loss_type in (0, 1):
        for B in rr.EXACT_SIZES:
            params, rows = rr.exact_case(D, W, B, loss_type)
            assert np.array_equal(params, np.round(params)) and np.array_equal(rows, np.round(rows))
            assert rr.exact_bound(params, D, W, rows, loss_type) < rr.LIMIT
            parts = {}
            out, num, loss, grad = rr.loss_and_grad(params, D, W, rows, loss_type, parts)
            assert np.array_equal(parts["gsum"], np.round(parts["gsum"])) and num == round(num)
            if B < 63:
                continue
            for (w, b), a in zip(rr.split(parts["gsum"], D, W), parts["acts"] + [None]):
                assert np.any(w != 0) and np.any(b != 0)
                assert a is None or (np.any(a > 0) and np.any(a == 0))
            d = parts["dout"]
            assert np.any(d > 0) and np.any(d < 0) and (loss_type == 0 or np.any(d == 0))
    # asymmetric matrices: a transposed operand reads other values
    params, _ = rr.exact_case(D, W, 64, 0)
    for w, _b in rr.split(params, D, W)[1:-1]:
        assert not np.array_equal(w, w.T) and set(np.unique(w)) == {-1.0, 0.0, 1.0} and np.all((w != 0).sum(axis=1) == 3)


def test_checkpoint_layout_loads_into_stock_modules():
    """optimizer_state_dict() is torch.optim.Adam's own layout: a stock Adam over a stock module chain loads it (no GPU: the
    state is built by hand, as save_checkpoint builds it)."""
    from lidarnerf.raydrop import RayDropMLP, RayDropTrainer
    torch.manual_seed(5)
    m = RayDropMLP(2, 128)
    tr = RayDropTrainer.__new__(RayDropTrainer)  # the host-side pieces only
    tr.model, tr.betas, tr.eps, tr.global_step = m, (0.9, 0.999), 1e-8, 7
    tr.lr_schedule = np.linspace(5e-4, 1e-4, 50)
    P = m.num_parameters
    tr.exp_avg, tr.exp_avg_sq = torch.randn(P), torch.rand(P)
    tr._steps, tr._cur = torch.tensor([0.0, 7.0]), 1
    sd = tr.optimizer_state_dict()
    stock = _stock(2, 128)
    stock.load_state_dict(m.state_dict())
    opt = torch.optim.Adam(stock.parameters(), lr=1.0)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == tr.lr_schedule[7] and opt.param_groups[0]["betas"] == (0.9, 0.999)
    o = 0
    for p in stock.parameters():
        st = opt.state[p]
        n = p.numel()
        assert float(st["step"]) == 7 and torch.equal(st["exp_avg"].reshape(-1), tr.exp_avg[o:o + n])
        assert torch.equal(st["exp_avg_sq"].reshape(-1), tr.exp_avg_sq[o:o + n]) and st["exp_avg"].shape == p.shape
        o += n
    # and the stock optimizer can step from it
    for p in stock.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert float(opt.state[next(iter(stock.parameters()))]["step"]) == 8
