"""Host side of the ray-drop U-Net's training step (csrc/unet_train_step.hip, lidarnerf/unet_train.py, lidarnerf/unet_trainer.py; DESIGN
§19): exports and signatures, every argument refusal (validation happens before any launch, so none needs a GPU), the size functions
against their Python twins, the float64 restatement (tests/unet_trainer_ref.py) against golden G18 and against the stock optimizer, the
problem with one answer, the scheduler against torch's, the optimizer state's layout, and the teeth of the loss bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import unet_ref as R
import unet_train_ref as T
import unet_trainer_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1  # LNH_ERR_INVALID_ARG (include/lidarnerf_hip.h)
NEW = ("lnh_unet_loss_grad", "lnh_unet_loss_grad_workspace_size", "lnh_unet_grad_sumsq", "lnh_unet_grad_sumsq_workspace_size",
       "lnh_unet_rmsprop_step")


def test_exports_header_and_signatures():
    from lidarnerf import _hip, unet_train, unet_trainer
    L = _hip.lib()
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(L, name) and name in text and name in unet_train._STEP_SYMBOLS, name
        assert _hip._OPTIONAL[name] == "U-Net training"
    assert len(_hip._SIGS["lnh_unet_loss_grad"]) == 9 and _hip._SIGS["lnh_unet_loss_grad"][3] is C.c_uint64
    assert len(_hip._SIGS["lnh_unet_grad_sumsq"]) == 5 and len(_hip._SIGS["lnh_unet_rmsprop_step"]) == 9
    assert _hip._SIGS["lnh_unet_rmsprop_step"][3:] == [C.c_double] * 6
    assert L.lnh_unet_loss_grad_workspace_size.restype is C.c_uint64 and L.lnh_unet_grad_sumsq_workspace_size.restype is C.c_uint64
    slots = ("LR", "STEP", "SKIPPED", "SUMSQ", "NORM", "COEF", "NONFINITE")
    for i, s in enumerate(slots):
        assert getattr(_hip, "URS_" + s) == i and f"#define LNH_URS_{s} {i}" in text, s
    assert f"#define LNH_URS_SLOTS {_hip.URS_SLOTS}" in text and f"#define LNH_URS_MAX_TENSORS {_hip.URS_MAX_TENSORS}" in text
    assert (_hip.UNET_MASK_F32, _hip.UNET_MASK_U8) == (0, 1) and "LNH_UNET_MASK_F32 0u" in text and "LNH_UNET_MASK_U8 1u" in text
    assert _hip.URS_TENSOR_WORDS == 5 and "typedef struct lnh_urs_tensor" in text
    for name in ("raydrop_unet_loss_and_grad", "loss_grad_workspace_bytes", "grad_sumsq", "grad_sumsq_workspace_bytes", "rmsprop_step",
                 "step_table"):
        assert callable(getattr(unet_train, name)), name
    for name in ("train_step", "evaluate", "scheduler_step", "train_epoch", "optimizer_state_dict", "load_optimizer_state_dict",
                 "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(unet_trainer.RayDropUNetTrainer, name)), name


def test_size_functions_are_their_python_twins():
    from lidarnerf import _hip, unet_train as ut
    L = _hip.lib()
    for M in (1, 63, 64, 65, 255, 256, 257, 773, 3072, 65535, 65536, 65537, 67980, 131073, 1 << 20, (1 << 26) - 1, 1 << 26):
        E, parts = ut.loss_grad_partials(M)
        assert L.lnh_unet_loss_grad_workspace_size(M) == ut.loss_grad_workspace_bytes(M) == parts * 24
        assert E % 256 == 0 and (parts - 1) * E < M <= parts * E and parts <= 256
    assert ut.loss_grad_partials(773) == (256, 4) and ut.loss_grad_partials(67980) == (512, 133)
    for M in (0, (1 << 26) + 1, 1 << 40):
        assert L.lnh_unet_loss_grad_workspace_size(M) == ut.loss_grad_workspace_bytes(M) == 0
    assert L.lnh_unet_grad_sumsq_workspace_size() == ut.grad_sumsq_workspace_bytes() == 8192


def test_every_argument_refusal():
    """Null and misaligned pointers, a dtype code that does not exist, M of 0 and beyond 2^26, a workspace one byte short, a table of 0
    or 65 tensors, every hyperparameter torch's RMSprop refuses: LNH_ERR_INVALID_ARG with a message, nothing launched (no pointer is
    dereferenced)."""
    from lidarnerf import _hip
    L = _hip.lib()
    p, big = 1 << 20, 1 << 30

    def err():
        return L.lnh_last_error().decode()

    def loss(x=p, t=p, dtype=0, M=100, scale=1.0, ws=p, wsb=big, out=p, d=p):
        return L.lnh_unet_loss_grad(x, t, dtype, M, scale, ws, wsb, out, d, None)

    for k in ("x", "t", "ws", "out", "d"):
        assert loss(**{k: None}) == INVALID_ARG and "unet_loss_grad: null" in err(), k
    assert loss(dtype=2) == INVALID_ARG and "mask_dtype" in err()
    for M in (0, (1 << 26) + 1):
        assert loss(M=M) == INVALID_ARG and "M =" in err()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert loss(scale=scale) == INVALID_ARG and "loss_scale" in err()
    assert loss(M=773, wsb=4 * 24 - 1) == INVALID_ARG and "workspace" in err()
    for kw in (dict(x=p + 2), dict(t=p + 2), dict(ws=p + 4), dict(out=p + 1), dict(d=p + 2)):
        assert loss(**kw) == INVALID_ARG and "aligned" in err(), kw
    assert loss(t=p + 1, dtype=2) == INVALID_ARG

    def sumsq(table=p, n=64, ws=p, wsb=8192, state=p):
        return L.lnh_unet_grad_sumsq(table, n, ws, wsb, state, None)

    def step(table=p, n=64, state=p, scale=1024.0, max_norm=1.0, alpha=0.99, eps=1e-8, wd=1e-8, momentum=0.999):
        return L.lnh_unet_rmsprop_step(table, n, state, scale, max_norm, alpha, eps, wd, momentum, None)

    for fn, who in ((sumsq, "unet_grad_sumsq"), (step, "unet_rmsprop_step")):
        for k in ("table", "state"):
            assert fn(**{k: None}) == INVALID_ARG and who + ": null" in err(), (who, k)
        for n in (0, 65, 1 << 20):
            assert fn(n=n) == INVALID_ARG and "n_tensors" in err(), (who, n)
        for k in ("table", "state"):
            assert fn(**{k: p + 4}) == INVALID_ARG and "aligned" in err(), (who, k)
    assert sumsq(ws=None) == INVALID_ARG and "workspace" in err() and sumsq(ws=p + 4) == INVALID_ARG and "workspace" in err()
    assert sumsq(wsb=8191) == INVALID_ARG and "workspace" in err()
    for scale in (0.0, -2.0, float("inf"), float("nan")):
        assert step(scale=scale) == INVALID_ARG and "loss_scale" in err()
    for max_norm in (0.0, -1.0, float("nan")):
        assert step(max_norm=max_norm) == INVALID_ARG and "max_norm" in err()
    for k in ("alpha", "eps", "wd", "momentum"):
        for v in (-1e-3, float("inf"), float("nan")):
            assert step(**{k: v}) == INVALID_ARG and {"wd": "weight_decay"}.get(k, k) in err(), (k, v)


def test_wrapper_refusals():
    from lidarnerf import unet_train as ut
    from lidarnerf.unet_trainer import RayDropUNetTrainer
    x = torch.zeros(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="f32"):
        ut.raydrop_unet_loss_and_grad(x.double(), x, x.clone(), torch.zeros(1), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="masks must be"):
        ut.raydrop_unet_loss_and_grad(x, x.long(), x.clone(), torch.zeros(1), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="elements"):
        ut.raydrop_unet_loss_and_grad(x, x[:1], x.clone(), torch.zeros(1), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        ut.raydrop_unet_loss_and_grad(x, x, x.clone(), torch.zeros(1), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="tensors"):
        ut.step_table([], [], [])
    with pytest.raises(RuntimeError, match="tensors"):
        ut.step_table([x] * 65, [x] * 65, [x] * 65)
    with pytest.raises(RuntimeError, match="one size"):
        ut.step_table([x], [x], [x])  # not on the GPU
    with pytest.raises(RuntimeError, match="int64"):
        ut.grad_sumsq(torch.zeros(5), 1, torch.zeros(8192, dtype=torch.uint8), torch.zeros(8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="float64"):
        ut.rmsprop_step(torch.zeros(1, 5, dtype=torch.int64), 1, torch.zeros(8))
    with pytest.raises(RuntimeError, match="int64"):
        ut.rmsprop_step(torch.zeros(1, 5, dtype=torch.int64), 2, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="momentum > 0 needs a table"):  # a table without the host-side note of its buffers
        ut.rmsprop_step(torch.zeros(1, 5, dtype=torch.int64), 1, torch.zeros(8, dtype=torch.float64), momentum=0.5)
    with pytest.raises(TypeError, match="RayDropUNet"):
        RayDropUNetTrainer(torch.nn.Linear(2, 2))


# ------------------------------------------------------------------------------------------------------ the loss in closed form
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g18_unet_loss.npz"))


@pytest.mark.parametrize("k", range(len(T.LOSS_CASES)))
def test_closed_form_equals_the_references_loss_and_gradient(k):
    g = _golden()
    x, t = (a.numpy() for a in T.loss_case(k))
    loss, grad = TR.loss_and_grad(x, t)
    assert abs(loss - float(g[f"loss64_{k}"])) < 1e-12
    assert float(np.abs(grad - g[f"grad64_{k}"]).max()) < 1e-12 and float(np.abs(grad).max()) > 0


@pytest.mark.parametrize("M", (1, 63, 65, 257))
def test_closed_form_equals_float64_autograd(M):
    from lidarnerf import unet_train as ut
    x, t = TR.hashed_loss_case(M, M)
    xt = torch.from_numpy(x).reshape(1, 1, M).requires_grad_(True)
    loss = ut.raydrop_unet_loss(xt, torch.from_numpy(t).reshape(1, 1, M))
    loss.backward()
    want_loss, want = TR.loss_and_grad(x, t, loss_scale=1024.0)
    assert abs(want_loss - loss.item()) < 1e-12 and float(np.abs(want / 1024 - xt.grad.numpy().reshape(M)).max()) < 1e-12


def test_closed_form_where_the_epsilon_or_the_empty_rule_decides():
    """Logits -15 on an empty 4 x 4 mask: S = 16 sigmoid(-15) = 4.9e-6, of the epsilon's size.  Logits -1000: S == 0 exactly (exp
    underflows in float64), dice = 1, no dice gradient.  Logits +-100, +-40 with both mask values: finite."""
    from lidarnerf import unet_train as ut
    x, t = np.full(16, -15.0), np.zeros(16)
    xt = torch.from_numpy(x).reshape(1, 4, 4).requires_grad_(True)
    loss = ut.raydrop_unet_loss(xt, torch.zeros(1, 4, 4, dtype=torch.float64))
    loss.backward()
    want_loss, want = TR.loss_and_grad(x, t)
    assert abs(want_loss - loss.item()) < 1e-12 and float(np.abs(want - xt.grad.numpy().reshape(16)).max()) < 1e-15
    # the epsilon decides the dice part here: without it, I = 0 and t = 0 leave no dice gradient at all
    assert TR.loss_terms(x, t)[2][0] > 1e-3 and TR.loss_terms(x, t, "no_eps")[2][0] == 0
    loss, g_bce, g_dice = TR.loss_terms(np.full(16, -1000.0), np.zeros(16))
    assert loss == 0.0 and not g_dice.any() and not g_bce.any()
    x = np.array([100.0, -100.0, 40.0, -40.0] * 2)
    t = np.array([0.0] * 4 + [1.0] * 4)
    loss, grad = TR.loss_and_grad(x, t)
    assert np.isfinite(loss) and np.isfinite(grad).all() and abs(grad[1] + 0) < 1e-40 and abs(grad[0] - 1 / 8) < 1e-3


BOUND_CASES = [T.loss_case(k) for k in range(len(T.LOSS_CASES))]


def _exceeds(variant):
    """Cases on which the wrong form `variant` leaves the GPU test's bound (loss or any gradient element)."""
    out = []
    cases = [(a.numpy().ravel(), b.numpy().ravel()) for a, b in BOUND_CASES]
    cases += [(np.full(16, -15.0), np.zeros(16)), (np.full(16, -1000.0), np.zeros(16)), (np.full(16, -200.0), np.zeros(16))]
    for i, (x, t) in enumerate(cases):
        want_loss, want = TR.loss_and_grad(x, t)
        b_loss, b = TR.loss_grad_bound(x, t)
        with np.errstate(all="ignore"):
            loss, grad = TR.loss_and_grad(x, t, variant=variant)
        if not (abs(loss - want_loss) <= b_loss and (np.abs(grad - want) <= b).all()):
            out.append(i)
    return out


def test_the_loss_bound_has_teeth_and_stays_under_its_ceiling():
    """The per-element bound of the GPU test is nowhere above 2^-18 (1 / M + |dice part|); the restatement itself is inside it; the
    dice epsilon dropped, 2 t taken as t and a missing 1 / M each leave it on at least one case.  PyTorch's own fp32 autograd of the
    same loss leaves it too: the bound is a demand on the float64 sums, not a formality."""
    from lidarnerf import unet_train as ut
    for x, t in BOUND_CASES:
        x, t = x.numpy().ravel(), t.numpy().ravel()
        for scale in (1.0, 1024.0):
            assert (TR.loss_grad_bound(x, t, scale)[1] <= TR.loss_grad_ceiling(x, t, scale)).all()
    assert _exceeds(None) == []
    for variant in ("no_eps", "t_not_2t", "no_1_over_M"):
        bad = _exceeds(variant)
        print(variant, "leaves the bound on cases", bad)
        assert bad, variant
    x, t = BOUND_CASES[0]
    x32 = x.float().requires_grad_(True)
    ut.raydrop_unet_loss(x32, t.float()).backward()
    want = TR.loss_and_grad(x.float().double().numpy(), t.numpy())[1]
    assert not (np.abs(x32.grad.double().numpy() - want) <= TR.loss_grad_bound(x.float().double().numpy(), t.numpy())[1]).all()


def test_the_empty_rule_alone_changes_nothing_and_carries_the_epsilon_free_form():
    """The issue lists "the S == 0 rule dropped" among the variants that must leave the bound.  With the epsilon in place it cannot:
    S == 0 means every s_i is exactly 0 (they are non-negative), so s_i (1 - s_i) = 0 and the dice part is 0 x finite = 0, and
    dice = (0 + e) / (0 + e) = 1 exactly — the rule and its absence give the same bits on every input, which this test asserts on the
    cases above (two of them with S == 0).  The rule is load-bearing only together with a zero epsilon, where its absence is 0 / 0:
    asserted as well.  (torch's masked_fill is there for the same reason: dice_coeff can be called with epsilon = 0.)"""
    assert _exceeds("no_empty_rule") == []
    x, t = np.full(16, -1000.0), np.zeros(16)
    a, b = TR.loss_and_grad(x, t), TR.loss_and_grad(x, t, variant="no_empty_rule")
    assert a[0] == b[0] == 0.0 and np.array_equal(a[1], b[1])
    e = np.exp(-np.abs(x))
    with np.errstate(all="ignore"):
        assert np.isnan(np.float64(2 * 0.0 + 0.0) / (np.sum(e / (1 + e) + t) + 0.0))  # epsilon and rule both dropped: 0 / 0


# ------------------------------------------------------------------------------------------------------ clip + RMSprop
def _stock_steps(params, step_grads, max_norm, dtype, **kw):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    opt = torch.optim.RMSprop(ps, foreach=True, **kw)
    norms = []
    for grads in step_grads:
        for p, g in zip(ps, grads):
            p.grad = g.to(dtype).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    return ps, opt, norms


def test_restated_clip_rmsprop_equals_torch_in_float64():
    """Three steps, hashed data, weight decay, momentum, the first step clipped (norm 37) and the others not: parameters, square_avg
    and momentum_buffer against clip_grad_norm_ + torch.optim.RMSprop(foreach=True) to 1e-12."""
    shapes = [(7,), (3, 5), (64,), (2, 3, 3, 3), (1,)]
    kw = dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-3, momentum=0.9)
    params = [torch.from_numpy(R.hash_u01(9950 + i, int(np.prod(s))) - 0.5).reshape(s) for i, s in enumerate(shapes)]
    step_grads = []
    for j in range(3):
        gs = [torch.from_numpy(R.hash_u01(9960 + 8 * j + i, int(np.prod(s))) - 0.5).reshape(s) for i, s in enumerate(shapes)]
        norm = sum(float((g ** 2).sum()) for g in gs) ** 0.5
        gs = [g * ((37.0 if j == 0 else 0.5) / norm) for g in gs]
        step_grads.append(gs)
    ps, opt, norms = _stock_steps(params, step_grads, 1.0, torch.float64, **kw)
    assert abs(norms[0] - 37.0) < 1e-9 and norms[1] < 1.0 and norms[2] < 1.0
    p, sq, buf = params, [torch.zeros_like(t) for t in params], [torch.zeros_like(t) for t in params]
    for j, gs in enumerate(step_grads):
        p, sq, buf, total, coef = TR.clip_rmsprop(p, [g * 1024 for g in gs], sq, buf, max_norm=1.0, loss_scale=1024.0, **kw)
        assert abs(total - norms[j]) < 1e-9 and (coef < 1.0) == (j == 0)
    for i in range(len(shapes)):
        st = opt.state[ps[i]]
        assert float((p[i] - ps[i].detach()).abs().max()) < 1e-12 and float((sq[i] - st["square_avg"]).abs().max()) < 1e-12
        assert float((buf[i] - st["momentum_buffer"]).abs().max()) < 1e-12


def test_the_exact_optimizer_problem_has_one_answer():
    """EXACT's settings and exact_problem's data: the stock fp32 optimizer, the restatement run in fp32 and the restatement in float64
    agree bit for bit over three steps; square_avg = g1^2 / 4 after every step; everything stays dyadic."""
    shapes = [(1,), (3,), (63,), (64,), (65,), (4, 5, 3, 3), (1025,)]
    params, steps = TR.exact_problem(shapes)
    ps, opt, _ = _stock_steps(params, steps, 2.0 ** 20, torch.float32, **TR.EXACT)
    for dtype in (torch.float32, torch.float64):
        p, sq, buf = [t.to(dtype) for t in params], [torch.zeros_like(t, dtype=dtype) for t in params], [torch.zeros_like(t, dtype=dtype) for t in params]
        for j in range(3):
            p, sq, buf, total, coef = TR.clip_rmsprop(p, [g.to(dtype) * 1024 for g in steps[j]], sq, buf, max_norm=2.0 ** 20, loss_scale=1024.0,
                                                      **TR.EXACT)
            assert coef == 1.0
            for i in range(len(shapes)):
                assert torch.equal(sq[i], (steps[0][i].to(dtype) ** 2) / 4), (j, i)
        for i in range(len(shapes)):
            st = opt.state[ps[i]]
            assert torch.equal(p[i].float(), ps[i].detach()) and torch.equal(sq[i].float(), st["square_avg"]), i
            assert torch.equal(buf[i].float(), st["momentum_buffer"]) and torch.equal(p[i] * 8, (p[i] * 8).round()), i
    assert sorted({float(v) for g in steps[0] for v in g.abs().unique()}) == [2.0 ** k for k in range(-3, 4)]
    assert all(torch.equal(steps[j][i].abs() * 2, steps[0][i].abs()) for j in (1, 2) for i in range(len(shapes)))


def test_scheduler_is_torchs_reduce_on_plateau():
    from lidarnerf.unet_trainer import plateau_state, plateau_step
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.RMSprop([w], lr=1e-5)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "max", patience=5)
    s, lr, lrs = plateau_state(), 1e-5, []
    for score in TR.plateau_scores():
        sched.step(score)
        lr = plateau_step(s, lr, score)
        lrs.append(lr)
        assert lr == opt.param_groups[0]["lr"] and s["best"] == sched.best and s["num_bad_epochs"] == sched.num_bad_epochs, score
    assert sorted(set(lrs), reverse=True) == [1e-5, 1e-5 * 0.1, 1e-5 * 0.1 * 0.1]  # two plateaus, two cuts
    assert plateau_step(plateau_state(), 1e-8, 0.0) == 1e-8
    s = plateau_state()
    lr = 5e-9
    for _ in range(8):
        lr = plateau_step(s, lr, 0.0)
    assert lr == 5e-9  # a cut of less than eps = 1e-8 is not made, as in torch


def test_optimizer_state_dict_is_torchs_layout():
    """rmsprop_state_dict (what RayDropUNetTrainer.optimizer_state_dict returns) loads into a stock RMSprop over the stock UNet's 64
    parameters, continues there, and the stock optimizer's own state_dict has the same keys."""
    from lidarnerf.unet_trainer import rmsprop_state_dict
    net = R.stock_unet()
    params = list(net.parameters())
    assert len(params) == 64
    hyper = dict(lr=1e-4, alpha=0.99, eps=1e-8, weight_decay=1e-8, momentum=0.999)
    sq = [torch.full_like(p, 0.25) for p in params]
    buf = [torch.full_like(p, -0.5) for p in params]
    sd = rmsprop_state_dict(3, sq, buf, **hyper)
    opt = torch.optim.RMSprop(params, foreach=True, **hyper)
    assert sd["param_groups"][0].keys() == opt.state_dict()["param_groups"][0].keys()
    opt.load_state_dict(sd)
    for p in params[:3] + params[-2:]:
        st = opt.state[p]
        assert float(st["step"]) == 3 and torch.equal(st["square_avg"], torch.full_like(p, 0.25))
        assert torch.equal(st["momentum_buffer"], torch.full_like(p, -0.5))
    back = opt.state_dict()
    assert sorted(back["state"]) == list(range(64)) and back["state"][0].keys() == sd["state"][0].keys()
    assert back["param_groups"][0]["params"] == list(range(64)) and back["param_groups"][0]["lr"] == 1e-4
    assert rmsprop_state_dict(0, sq, buf, **hyper)["state"] == {}
    assert "momentum_buffer" not in rmsprop_state_dict(1, sq[:2], buf[:2], **dict(hyper, momentum=0.0))["state"][0]
