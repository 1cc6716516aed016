"""Host side of U-Net training (lidarnerf/unet_train.py, csrc/unet_train.hip): exports, signatures and every argument
refusal of the backward entry points (pool, head, transposed convolution: pack, data gradient, weight gradient), their workspace
sizes, the loss and the validation score against the reference's recorded values
(golden G18), and the float64 restatement of tests/unet_train_ref.py — which the kernel tests of tests/test_unet_train_gpu.py are held
to — against autograd of the stock modules, with the conditions that make those kernel tests exact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
import unet_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1  # LNH_ERR_INVALID_ARG (include/lidarnerf_hip.h)


def test_exports_and_signatures():
    from lidarnerf import _hip, unet_train
    L = _hip.lib()
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    for name in ("lnh_unet_pool_backward", "lnh_unet_head_backward", "lnh_unet_head_backward_workspace_size", "lnh_unet_pack_upconv",
                 "lnh_unet_upconv2x2_backward_data", "lnh_unet_upconv2x2_backward_weight",
                 "lnh_unet_upconv2x2_backward_weight_workspace_size"):
        assert name in _hip.EXPORTS and hasattr(L, name) and name in text and name in unet_train._SYMBOLS, name
    assert len(_hip._SIGS["lnh_unet_pool_backward"]) == 9 and len(_hip._SIGS["lnh_unet_head_backward"]) == 11
    assert L.lnh_unet_head_backward_workspace_size.restype is C.c_uint64
    assert len(_hip._SIGS["lnh_unet_pack_upconv"]) == 5 and len(_hip._SIGS["lnh_unet_upconv2x2_backward_data"]) == 12
    assert len(_hip._SIGS["lnh_unet_upconv2x2_backward_weight"]) == 15
    assert L.lnh_unet_upconv2x2_backward_weight_workspace_size.restype is C.c_uint64


def test_head_workspace_size_is_its_python_twin():
    from lidarnerf import _hip, unet_train
    L = _hip.lib()
    for N, H, W in ((1, 1, 1), (1, 1, 64), (1, 5, 13), (2, 17, 19), (2, 66, 1030), (64, 1024, 1024)):
        want = (N * H * W + 63) // 64 * 65 * 4
        assert L.lnh_unet_head_backward_workspace_size(N, H, W) == unet_train.head_backward_workspace_bytes(N, H, W) == want
    for N, H, W in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (65, 1024, 1024)):
        assert L.lnh_unet_head_backward_workspace_size(N, H, W) == 0


def test_upconv_weight_workspace_size_is_its_python_twin():
    """The slices are a function of the shape: the top level of a 66 x 1030 frame is split, the deepest is not, no workspace passes
    16 MiB + one slice; the exact tests' shapes have one slice and two."""
    from lidarnerf import _hip, unet_train as ut
    L = _hip.lib()
    for N, H, W, Cin, Cout in ((1, 1, 2, 128, 64), (1, 4, 64, 128, 64), (2, 9, 17, 128, 64), (1, 9, 17, 1024, 512), (1, 33, 515, 128, 64),
                               (2, 33, 515, 128, 64), (1, 4, 64, 1024, 512), (2, 8, 128, 512, 256), (1, 1024, 1024, 1024, 1024)):
        S, Lp = ut.upconv_wgrad_slices(N * H * W, Cin, Cout)
        want = S * (4 * Cin * Cout + Cout) * 4
        assert L.lnh_unet_upconv2x2_backward_weight_workspace_size(N, H, W, Cin, Cout) == want == \
            ut.upconv2x2_backward_weight_workspace_bytes(N, H, W, Cin, Cout)
        assert Lp % 32 == 0 and (S - 1) * Lp < N * H * W <= S * Lp and want <= (16 << 20) + (4 * Cin * Cout + Cout) * 4
    assert ut.upconv_wgrad_slices(33 * 515, 128, 64)[0] == 67 and ut.upconv_wgrad_slices(4 * 64, 1024, 512) == (1, 256)
    assert ut.upconv_wgrad_slices(306, 128, 64) == (2, 160) and ut.upconv_wgrad_slices(153, 1024, 512)[0] == 1
    for shape in ((0, 4, 4, 128, 64), (1, 0, 4, 128, 64), (1, 4, 4, 32, 64), (1, 4, 4, 96, 64), (1, 4, 4, 128, 32), (1, 4, 4, 1088, 64),
                  (1, 4096, 4097, 128, 64)):
        assert L.lnh_unet_upconv2x2_backward_weight_workspace_size(*shape) == 0


def test_every_argument_refusal_of_the_entry_points():
    """Validation happens before any launch, so it runs without a GPU (the pointers are never dereferenced)."""
    from lidarnerf import _hip
    L = _hip.lib()
    p = 1 << 20

    def err():
        return L.lnh_last_error().decode()

    def pool(x=p, N=1, H0=7, W0=9, Cc=64, dpool=p, dskip=None, stride=0, dx=p):
        return L.lnh_unet_pool_backward(x, N, H0, W0, Cc, dpool, dskip, stride, dx, None)

    for kw in (dict(x=None), dict(dpool=None), dict(dx=None)):
        assert pool(**kw) == INVALID_ARG and "null" in err()
    for Cc in (0, 8, 48, 1056):
        assert pool(Cc=Cc) == INVALID_ARG and "C " in err()
    for kw in (dict(N=0), dict(H0=1), dict(W0=1), dict(N=1 << 12, H0=1 << 10, W0=1 << 10)):
        assert pool(**kw) == INVALID_ARG and "source" in err()
    for kw in (dict(stride=64), dict(dskip=p, stride=0), dict(dskip=p, stride=32), dict(dskip=p, stride=68), dict(dskip=p, stride=2056)):
        assert pool(**kw) == INVALID_ARG and "stride" in err()
    for kw in (dict(x=p + 8), dict(dpool=p + 8), dict(dx=p + 8), dict(dskip=p + 8, stride=64)):
        assert pool(**kw) == INVALID_ARG and "aligned" in err()

    big = 1 << 30

    def head(a=p, N=2, H=17, W=19, w=p, d=p, ws=p, wsb=big, dx=p, dw=p, db=p):
        return L.lnh_unet_head_backward(a, N, H, W, w, d, ws, wsb, dx, dw, db, None)

    for k in ("a", "w", "d", "ws", "dx", "dw", "db"):
        assert head(**{k: None}) == INVALID_ARG and "null" in err(), k
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(N=65, H=1024, W=1024)):
        assert head(**kw) == INVALID_ARG and "image" in err()
    assert head(wsb=11 * 65 * 4 - 1) == INVALID_ARG and "workspace" in err()  # 646 pixels: 11 waves
    for k in ("a", "w", "ws", "dx"):
        assert head(**{k: p + 8}) == INVALID_ARG and "aligned" in err(), k


def test_every_argument_refusal_of_the_transposed_convolution_entry_points():
    from lidarnerf import _hip
    L = _hip.lib()
    p = 1 << 20

    def err():
        return L.lnh_last_error().decode()

    def pack(w=p, Cin=128, Cout=64, fwd=p, bwd=p):
        return L.lnh_unet_pack_upconv(w, Cin, Cout, fwd, bwd, None)

    assert pack(w=None) == INVALID_ARG and "null" in err() and pack(fwd=None) == INVALID_ARG and "null" in err()
    for Cin in (0, 32, 96, 1088):
        assert pack(Cin=Cin) == INVALID_ARG and "Cin" in err()
    for Cout in (0, 32, 96, 1088):
        assert pack(Cout=Cout) == INVALID_ARG and "Cout" in err()
    for kw in (dict(w=p + 4), dict(fwd=p + 2), dict(bwd=p + 8)):
        assert pack(**kw) == INVALID_ARG and "aligned" in err()

    def data(dy=p, Hd=8, Wd=10, stride=64, off=0, N=1, H=4, W=5, Cin=128, Cout=64, w=p, dx=p):
        return L.lnh_unet_upconv2x2_backward_data(dy, Hd, Wd, stride, off, N, H, W, Cin, Cout, w, dx, None)

    for kw in (dict(dy=None), dict(w=None), dict(dx=None)):
        assert data(**kw) == INVALID_ARG and "null" in err()
    for Cin in (0, 32, 96, 1088):
        assert data(Cin=Cin) == INVALID_ARG and "Cin" in err()
    for Cout in (0, 16, 48, 1056):
        assert data(Cout=Cout, stride=2048) == INVALID_ARG and "Cout" in err()
    for kw in (dict(N=0), dict(H=0, Hd=0), dict(N=1 << 10, H=1 << 10, W=1 << 5, Hd=1 << 11, Wd=1 << 6)):
        assert data(**kw) == INVALID_ARG and "image" in err()
    for Hd, Wd in ((7, 10), (10, 10), (8, 9), (8, 12)):
        assert data(Hd=Hd, Wd=Wd) == INVALID_ARG and "larger" in err()
    for kw in (dict(stride=60), dict(stride=68, off=4), dict(stride=64, off=8), dict(stride=2056), dict(stride=32)):
        assert data(**kw) == INVALID_ARG and "per pixel" in err()
    for kw in (dict(dy=p + 8), dict(w=p + 8), dict(dx=p + 8)):
        assert data(**kw) == INVALID_ARG and "aligned" in err()

    def wgt(x=p, dy=p, Hd=8, Wd=10, stride=64, off=0, N=1, H=4, W=5, Cin=128, Cout=64, ws=p, wsb=1 << 30, dw=p, db=p):
        return L.lnh_unet_upconv2x2_backward_weight(x, dy, Hd, Wd, stride, off, N, H, W, Cin, Cout, ws, wsb, dw, db, None)

    for k in ("x", "dy", "ws", "dw", "db"):
        assert wgt(**{k: None}) == INVALID_ARG and "null" in err(), k
    for Cin in (0, 32, 96, 1088):
        assert wgt(Cin=Cin) == INVALID_ARG and "Cin" in err()
    for Cout in (0, 32, 96, 1088):
        assert wgt(Cout=Cout, stride=2048) == INVALID_ARG and "Cout" in err()
    for kw in (dict(N=0), dict(H=0, Hd=0), dict(N=1 << 10, H=1 << 10, W=1 << 5, Hd=1 << 11, Wd=1 << 6)):
        assert wgt(**kw) == INVALID_ARG and "image" in err()
    for Hd, Wd in ((7, 10), (10, 10), (8, 9), (8, 12)):
        assert wgt(Hd=Hd, Wd=Wd) == INVALID_ARG and "larger" in err()
    for kw in (dict(stride=60), dict(stride=72, off=4), dict(stride=64, off=8), dict(stride=2056), dict(stride=32)):
        assert wgt(**kw) == INVALID_ARG and "per pixel" in err()
    assert wgt(wsb=(4 * 128 * 64 + 64) * 4 - 1) == INVALID_ARG and "workspace" in err()
    for k in ("x", "dy", "ws"):
        assert wgt(**{k: p + 8}) == INVALID_ARG and "aligned" in err(), k


def test_wrapper_refusals():
    from lidarnerf import unet_train as ut
    h = torch.zeros(1, 4, 4, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.pool_backward(h, h[:, :2, :2].contiguous(), h)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.head_backward(h, torch.zeros(64, dtype=torch.float16), torch.zeros(1, 1, 4, 4), torch.zeros(65), h, torch.zeros(64),
                         torch.zeros(1))
    with pytest.raises(RuntimeError, match="GPU"):
        ut.pack_upconv(torch.zeros(128, 64, 2, 2), torch.zeros(4, 64, 128, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="GPU"):
        ut.upconv2x2_backward_data(torch.zeros(1, 8, 8, 64, dtype=torch.float16), torch.zeros(64, 4, 64, dtype=torch.float16), h)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.upconv2x2_backward_weight(h, torch.zeros(1, 8, 8, 64, dtype=torch.float16), torch.zeros(1 << 16), torch.zeros(64, 64, 2, 2),
                                     torch.zeros(64))


def test_kernel_problems_are_exact():
    """What makes torch.equal the right comparison in tests/test_unet_train_gpu.py: every value of the pool problems is an fp16 number
    and so is every route + skip sum; the head's sums of |products| stay below 2^24 in quarter units, so fp32 adds them exactly in
    any order; the cases cover odd sizes, ties, a zero plane, skip tensors as wide as C and wider, one wave - 1 / one wave / several."""
    for k, (N, Cc, H0, W0, Cs) in enumerate(T.POOL_CASES):
        c = T.pool_case(k)
        assert torch.equal(c["want"], R.q16(c["want"])) and torch.equal(c["dpool"], R.q16(c["dpool"]))
        assert not bool(c["x"][0, 0].any()) and c["want"].shape == (N, Cc, H0, W0)
        if H0 > 2:
            win = F.unfold(c["x"][:, :, :H0 // 2 * 2, :W0 // 2 * 2], 2, stride=2).reshape(N, Cc, 4, -1)
            assert float((win == win.max(2, keepdim=True).values).double().sum(2).mean()) > 1.3  # ties are the rule
    assert {c[4] == 0 for c in T.POOL_CASES} == {True, False} and any(c[4] > c[1] for c in T.POOL_CASES)
    assert any(c[2] % 2 and c[3] % 2 for c in T.POOL_CASES)
    for k, (N, H, W) in enumerate(T.HEAD_CASES):
        c = T.head_backward_case(k)
        assert 4 * c["bound"] < 2 ** 24 and torch.equal(c["want_dx"], R.q16(c["want_dx"]))
        assert torch.equal(c["want_dweight"], c["want_dweight"].float().double()) and c["want_dweight"].unique().numel() > 8
    assert {N * H * W for N, H, W in T.HEAD_CASES} >= {64, 65, 646}
    assert len(T.UPCONV_BWD_EMBED) == len(R.UPCONV_CASES)
    for k in range(len(R.UPCONV_CASES)):
        c = T.upconv_backward_case(k)
        assert c["bound"] < 2 ** 24 and c["want_dx"].unique().numel() > 20
        assert c["bound_w"] < 2 ** 24 and c["want_dweight"].unique().numel() > 8 and bool(c["want_dbias"].any())
        xw = c["weight"].clone().requires_grad_(True)  # dweight and dbias are conv_transpose2d's parameter gradients
        xb = torch.zeros(c["dy"].shape[1], dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(c["x"], xw, xb, stride=2).backward(c["dy"])
        assert torch.equal(xw.grad, c["want_dweight"]) and torch.equal(xb.grad, c["want_dbias"])
        x = torch.zeros_like(c["want_dx"]).requires_grad_(True)  # the formula is conv_transpose2d's input gradient
        F.conv_transpose2d(x, c["weight"], stride=2).backward(c["dy"])
        assert torch.equal(x.grad, c["want_dx"])
    assert {e[:2] for e in T.UPCONV_BWD_EMBED} == {(0, 0), (1, 0), (0, 1), (1, 1)}


# ------------------------------------------------------------------------------------------------------ loss and validation score (G18)
def _g18():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_unet_loss.npz"))


@pytest.mark.parametrize("k", range(len(T.LOSS_CASES)))
def test_loss_and_dice_are_the_references(k):
    """raydrop_unet_loss, its gradient, dice_coeff and the validation score against the values the reference's own functions gave
    (golden G18): 1e-12 in float64, float32 within 1e-6 of the reference's float32."""
    from lidarnerf import unet_train as ut
    g = _g18()
    logits, masks = T.loss_case(k)
    x = logits.clone().requires_grad_(True)
    loss = ut.raydrop_unet_loss(x[:, None], masks.to(torch.int64))  # [N, 1, H, W] logits, integer masks: the loop's types
    loss.backward()
    assert abs(loss.item() - float(g[f"loss64_{k}"])) < 1e-12
    assert float((x.grad - torch.from_numpy(g[f"grad64_{k}"])).abs().max()) < 1e-12 and float(x.grad.abs().max()) > 0
    assert abs(float(ut.raydrop_unet_loss(logits.float(), masks.float())) - float(g[f"loss32_{k}"])) < 1e-6
    assert abs(float(ut.raydrop_unet_dice_score(logits[:, None], masks)) - float(g[f"dice_eval64_{k}"])) < 1e-12
    assert abs(float(ut.dice_coeff(torch.sigmoid(logits), masks, reduce_batch_first=True)) - float(g[f"dice_soft64_{k}"])) < 1e-12
    assert abs(float(ut.dice_loss(torch.sigmoid(logits), masks)) - (1 - float(g[f"dice_soft64_{k}"]))) < 1e-12


def test_dice_of_empty_sets_and_refusals():
    from lidarnerf import unet_train as ut
    g = _g18()
    assert float(g["dice_eval64_3"]) == 1.0 and 1 / 3 < float(g["dice_eval64_2"]) < 1  # empty pairs score 1, as in the reference
    zero = torch.zeros(2, 4, 4, dtype=torch.float64)
    assert float(ut.dice_coeff(zero, zero)) == 1.0 and float(ut.dice_coeff(zero[0], zero[0])) == 1.0
    one = torch.ones(2, 4, 4, dtype=torch.float64)
    assert abs(float(ut.dice_coeff(one, one)) - 1.0) < 1e-12 and float(ut.dice_coeff(one, zero)) < 1e-6
    with pytest.raises(ValueError, match="differ"):
        ut.dice_coeff(zero, zero[:1])
    with pytest.raises(ValueError, match="reduce_batch_first"):
        ut.dice_coeff(zero[0], zero[0], reduce_batch_first=True)
    with pytest.raises(ValueError, match="logits must be"):
        ut.raydrop_unet_loss(torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4))
    with pytest.raises(ValueError, match="do not fit"):
        ut.raydrop_unet_loss(torch.zeros(2, 1, 4, 4), torch.zeros(2, 4, 5))


# ------------------------------------------------------------------------------------------------------ the whole net, float64
def test_pool_backward_is_torchs_with_ties_and_odd_sizes():
    """Integer inputs 0 .. 3 (most windows tie), odd sizes, with and without a skip gradient: equal to autograd of max_pool2d, which
    routes to the first maximum."""
    for k, shape in enumerate(((2, 3, 7, 9), (1, 4, 16, 17), (1, 2, 5, 4))):
        x = R.integer_image(9700 + k, shape).double().requires_grad_(True)
        dpool = (R.integer_image(9710 + k, shape[:2] + (shape[2] // 2, shape[3] // 2), top=4) - 2).double()
        F.max_pool2d(x, 2).backward(dpool)
        assert torch.equal(T.pool_backward(x.detach(), dpool), x.grad)
        dskip = R.integer_image(9720 + k, shape).double()
        assert torch.equal(T.pool_backward(x.detach(), dpool, dskip), x.grad + dskip)
        assert not bool(x.grad[:, :, 2 * (shape[2] // 2):].any()) and not bool(x.grad[:, :, :, 2 * (shape[3] // 2):].any())
    x = R.integer_image(9730, (1, 2, 6, 6)).double()  # a NaN takes over from any earlier value and is not displaced: torch's rule
    x[0, 0, 0, 1] = x[0, 0, 2, 2] = x[0, 1, 5, 5] = x[0, 1, 4, 4] = float("nan")
    x.requires_grad_(True)
    dpool = torch.arange(1.0, 19.0, dtype=torch.float64).reshape(1, 2, 3, 3)
    F.max_pool2d(x, 2).backward(dpool)
    assert torch.equal(T.pool_backward(x.detach(), dpool), x.grad) and x.grad[0, 0, 0, 1] == 1 and x.grad[0, 1, 5, 5] == 18
    zeros = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    assert torch.equal(T.pool_backward(zeros, torch.ones(1, 1, 2, 2, dtype=torch.float64))[0, 0],
                       torch.tensor([[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]], dtype=torch.float64))


def test_whole_net_training_restatement_is_autograd_of_the_stock_net():
    """unet_train_forward / unet_backward_from_state (no autograd inside) against the stock modules in training mode, float64, hashed
    weights, 2 x 23 x 37 (odd sizes: every level pads its upsampled tensor): logits to 1e-10, every parameter gradient to 1e-9 relative
    L2, the running statistics after the call to 1e-12; and the backward is linear in dlogits."""
    sd = R.hash_state_dict()
    x = torch.cat([R.g17_image(0), R.hash_input(1234, 1, 10, 23, 37)])
    stock = R.stock_unet().double().train()
    stock.load_state_dict(sd)
    logits = stock(x.double())
    dlogits = torch.from_numpy(np.where(R.hash_u01(9800, logits.numel()) < 0.5, -1.0, 1.0).reshape(logits.shape))
    logits.backward(dlogits)
    got, state = T.unet_train_forward(sd, x)
    assert float((got - logits.detach()).abs().max()) < 1e-10
    grads = T.unet_backward_from_state(sd, state, dlogits)
    params = dict(stock.named_parameters())
    assert set(grads) == set(params) and len(grads) == 18 * 3 + 8 + 2
    for name, p in params.items():
        rel = float((grads[name] - p.grad).norm() / p.grad.norm())
        assert grads[name].shape == p.grad.shape and rel < 1e-9, (name, rel)
    buffers = dict(stock.named_buffers())
    for name, v in state["running"].items():
        assert float((v - buffers[name]).abs().max()) < 1e-12, name
    assert len(state["running"]) == 36 and int(buffers["inc.double_conv.1.num_batches_tracked"]) == 1
    twice = T.unet_backward_from_state(sd, state, 2 * dlogits)
    assert float((twice["inc.double_conv.0.weight"] - 2 * grads["inc.double_conv.0.weight"]).abs().max()) < 1e-12


def test_restatement_equals_the_references_training_mode_record():
    """unet_train_forward / unet_backward_from_state against golden G18's record of the reference's own UNet in train() mode
    (g18_unet_train.npz): logits and the recorded running statistics to 1e-9, the recorded gradient norms to 1e-9 relative; the maker
    asserted the same for all 64 gradient tensors element by element (`dev_backward`)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_unet_train.npz"))
    sd = R.hash_state_dict()
    logits, state = T.unet_train_forward(sd, T.g18_train_batch())
    assert logits.shape == (2, 1, 23, 37) and float((logits - torch.from_numpy(g["logits64"])).abs().max()) < 1e-9
    for name in T.G18_RUNNING:
        assert float((state["running"][name] - torch.from_numpy(g[f"running_{name}"])).abs().max()) < 1e-9, name
    grads = T.unet_backward_from_state(sd, state, T.g18_train_cotangent())
    for name in T.G18_GRAD_NORMS:
        want = float(g[f"grad_norm_{name}"])
        assert want > 0 and abs(float(grads[name].norm()) - want) < 1e-9 * want, name
    assert float(g["dev_backward"]) < 1e-9 and 0 < float(g["dev_amp16"]) < 0.1 * float(g["std"])


@pytest.mark.parametrize("name", list(T.G18_BLOCKS))
def test_block_restatement_equals_the_references_blocks(name):
    """block_train against golden G18's records of the reference's DoubleConv / Down / Up / OutConv in train() mode, N = 2, 17 x 19:
    float64 outputs and running statistics to 1e-9; parameter and input gradients, stored rounded to float32, to 1e-7 relative L2
    (float32 holds 2^-24 per element; the maker asserted 1e-9 before rounding); the reference's own fp16-autocast deviation of every
    gradient is below 0.1."""
    golden = os.path.join(ROOT, "tests", "golden")
    g, gg = np.load(os.path.join(golden, f"g18_unet_block_{name}.npz")), np.load(os.path.join(golden, f"g18_unet_block_{name}_grads.npz"))
    sd = R.hash_state_dict()
    prefix = T.G18_BLOCKS[name][0]
    bsd = {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}
    out, backward, running = T.block_train(name, bsd, T.g18_block_inputs(name))
    want = torch.from_numpy(g["out64"])
    assert out.shape == want.shape and float((out - want).abs().max()) < 1e-9
    for k, v in running.items():
        assert float((v - torch.from_numpy(g[f"running_{k}"])).abs().max()) < 1e-9, k
    grads, dins = backward(T.g18_block_cotangent(name, out.shape))
    assert set(grads) == set(gg.files)
    for k, v in grads.items():
        w = torch.from_numpy(gg[k]).double()
        assert v.shape == w.shape and float((v - w).norm() / w.norm()) < 1e-7, k
        assert 0 <= float(g[f"dev_amp16_{k}"]) < 0.1
    for i, v in enumerate(dins):
        w = torch.from_numpy(g[f"dinput_{i}"]).double()
        assert v.shape == w.shape and float((v - w).norm() / w.norm()) < 1e-7 and float(g[f"dev_amp16_dinput_{i}"]) < 0.1
    if name == "up":
        assert out.shape == (2, 64, 17, 19) and len(dins) == 2 and dins[0].shape == (2, 128, 8, 9)


def test_loss_in_the_references_training_loop():
    """The shipped raydrop_unet_loss in the loop golden G18 recorded from the reference (g18_unet_record.npz): the stock net in float32
    with the hashed weights, the record's batch, RMSprop(lr 1e-4, momentum 0.999, weight decay 1e-8, foreach) and clip_grad_norm_(1).
    The first loss equals the reference's to float32 rounding of the same sums (1e-5); the next two stay within 2 x dev_loss, the
    gap the reference's own fp16-autocast run leaves (the bound the GPU learning test is to use).  The record itself: 16 steps, both
    runs fall below a tenth of their first loss."""
    from lidarnerf import unet_train as ut
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_unet_record.npz"))
    loss32, loss_amp, dev = g["loss32"], g["loss_amp"], float(g["dev_loss"])
    assert len(loss32) == len(loss_amp) == T.G18_STEPS and dev == float(np.abs(loss32 - loss_amp).max()) < 0.01
    assert loss32[-1] < 0.1 * loss32[0] and loss_amp[-1] < 0.1 * loss_amp[0]
    images, masks = T.g18_record_batch()
    assert 0.2 < float(masks.mean()) < 0.8
    torch.manual_seed(0)
    net = R.stock_unet().train()
    net.load_state_dict(R.hash_state_dict())
    opt = torch.optim.RMSprop(net.parameters(), lr=1e-4, momentum=0.999, weight_decay=1e-8, foreach=True)
    for step in range(3):
        loss = ut.raydrop_unet_loss(net(images), masks)
        assert abs(loss.item() - loss32[step]) <= (1e-5 if step == 0 else 2 * dev), (step, loss.item(), loss32[step])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
