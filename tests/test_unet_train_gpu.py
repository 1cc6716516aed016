"""The U-Net training kernels on the device (csrc/unet_train.hip through lidarnerf/unet_train.py) against the float64 restatement of
tests/unet_train_ref.py, in the habits of tests/test_unet_gpu.py: every output NaN-filled before the call and followed by guard words,
every call made twice with equal bits.  All comparisons are torch.equal on problems whose every value and sum is exact
(tests/test_unet_train_cpu.py asserts the conditions); no tolerance comes from the device's output."""
import pytest
import torch

import test_unet_gpu as G
import unet_ref as R
import unet_train_ref as T

pytestmark = pytest.mark.gpu


def _nhwc(x):
    """float64 NCHW on the host -> fp16 NHWC on the device, no channel padding."""
    return x.permute(0, 2, 3, 1).to(torch.float16).contiguous().cuda()


@pytest.mark.parametrize("k", range(len(T.POOL_CASES)))
def test_pool_backward_exact(k):
    """Ties, a zero plane, odd sizes (rows and columns no window covers get the skip gradient alone, or zero), without a skip and with
    one read in place from a tensor of C and of more channels per pixel."""
    from lidarnerf import unet_train as ut
    N, C, H0, W0, Cs = T.POOL_CASES[k]
    c = T.pool_case(k)
    x, dpool = _nhwc(c["x"]), _nhwc(c["dpool"])
    dskip = _nhwc(c["dskip"]) if Cs else None
    want = c["want"].permute(0, 2, 3, 1).contiguous().cuda()
    outs = []
    for _ in range(2):
        dx, guard = G.guarded((N, H0, W0, C), torch.float16)
        ut.pool_backward(x, dpool, dx, dskip)
        assert torch.equal(dx.double(), want), int((dx.double() != want).sum())
        assert G.guard_ok(guard)
        outs.append(dx)
    assert torch.equal(G._bits(outs[0]), G._bits(outs[1]))
    if not Cs:
        assert not bool(outs[0][:, 2 * (H0 // 2):].any()) and not bool(outs[0][:, :, 2 * (W0 // 2):].any())
        assert int((outs[0] != 0).sum()) <= dpool.numel()  # one owner per window


@pytest.mark.parametrize("k", range(len(T.HEAD_CASES)))
def test_head_backward_exact(k):
    """64, 65 and 646 pixels and more: one wave, one wave + 1 pixel, several waves with a ragged last one; the workspace NaN-filled."""
    from lidarnerf import unet_train as ut
    N, H, W = T.HEAD_CASES[k]
    c = T.head_backward_case(k)
    a, w = _nhwc(c["a"]), c["weight"].to(torch.float16).cuda()
    d = c["dlogits"].float().cuda()
    outs = []
    for _ in range(2):
        dx, g0 = G.guarded((N, H, W, 64), torch.float16)
        dw, g1 = G.guarded((1, 64, 1, 1), torch.float32)
        db, g2 = G.guarded((1,), torch.float32)
        ws, g3 = G.guarded((ut.head_backward_workspace_bytes(N, H, W) // 4,), torch.float32)
        ut.head_backward(a, w, d, ws, dx, dw, db)
        assert torch.equal(dx.double(), c["want_dx"].permute(0, 2, 3, 1).contiguous().cuda())
        assert torch.equal(dw.double().reshape(64), c["want_dweight"].cuda()) and torch.equal(db.double(), c["want_dbias"].cuda())
        assert all(G.guard_ok(g) for g in (g0, g1, g2, g3))
        outs.append((dx, dw, db))
    for p, q in zip(*outs):
        assert torch.equal(G._bits(p), G._bits(q))


def test_head_backward_passes_non_finite_dlogits_through():
    """Loss scaling is the caller's: an inf in dlogits gives a non-finite dbias and dweight (what GradScaler looks for) and non-finite
    dx at that pixel only; nothing is written outside the outputs."""
    from lidarnerf import unet_train as ut
    N, H, W = T.HEAD_CASES[0]
    c = T.head_backward_case(0)
    a, w = _nhwc(c["a"] + 1), c["weight"].to(torch.float16).cuda()
    d = c["dlogits"].float().cuda()
    d[1, 0, 3, 4] = float("inf")
    dx, g0 = G.guarded((N, H, W, 64), torch.float16)
    dw, g1 = G.guarded((64,), torch.float32)
    db, g2 = G.guarded((1,), torch.float32)
    ws, g3 = G.guarded((ut.head_backward_workspace_bytes(N, H, W) // 4,), torch.float32)
    ut.head_backward(a, w, d, ws, dx, dw, db)
    torch.cuda.synchronize()
    assert all(G.guard_ok(g) for g in (g0, g1, g2, g3))
    assert not bool(torch.isfinite(db).any()) and not bool(torch.isfinite(dw).any())
    bad = ~torch.isfinite(dx)
    assert bool(bad[1, 3, 4][w != 0].all()) and int(bad.sum()) == int(bad[1, 3, 4].sum())


@pytest.mark.parametrize("k", range(len(R.UPCONV_CASES)))
def test_upconv_pack_and_data_gradient_exact(k):
    """The images packed on the device from the fp32 parameter equal lidarnerf.unet's torch packing (forward) and its transpose
    (backward); dx is exact on unet_ref.UPCONV_CASES with dy read in place from a wider, taller gradient tensor whose other values
    are 3: 128 -> 64 and 1024 -> 512, 2 to 153 input pixels, N = 1 and 2, every combination of a padded row / column."""
    from lidarnerf import unet_train as ut
    Cin, Cout, H, W, N = R.UPCONV_CASES[k]
    c = T.upconv_backward_case(k)
    w32 = c["weight"].float().cuda()
    fwd, g0 = G.guarded((4, Cout, Cin), torch.float16)
    bwd, g1 = G.guarded((Cin, 4, Cout), torch.float16)
    ut.pack_upconv(w32, fwd, bwd)
    want_fwd = w32.permute(2, 3, 1, 0).reshape(4, Cout, Cin).to(torch.float16)
    assert torch.equal(fwd, want_fwd) and torch.equal(bwd, want_fwd.permute(2, 0, 1)) and G.guard_ok(g0) and G.guard_ok(g1)
    only, g2 = G.guarded((4, Cout, Cin), torch.float16)
    ut.pack_upconv(w32, only)
    assert torch.equal(only, want_fwd) and G.guard_ok(g2)
    dcat = _nhwc(c["dcat"])
    want = R.q16(c["want_dx"]).permute(0, 2, 3, 1).contiguous().cuda()  # (the one rounding: the fp16 store)
    outs = []
    for _ in range(2):
        dx, guard = G.guarded((N, H, W, Cin), torch.float16)
        ut.upconv2x2_backward_data(dcat, bwd, dx, offset=c["front"])
        assert torch.equal(dx.double(), want), int((dx.double() != want).sum())
        assert G.guard_ok(guard)
        outs.append(dx)
    assert torch.equal(G._bits(outs[0]), G._bits(outs[1]))


@pytest.mark.parametrize("k", range(len(R.UPCONV_CASES)))
def test_upconv_weight_and_bias_gradient_exact(k):
    """dweight in the parameter's [Cin, Cout, 2, 2] layout and dbias on unet_ref.UPCONV_CASES — 2, 18, 153, 256 and 306 input pixels
    (a ragged 32-pixel step, one slice, two slices), 128 -> 64 and 1024 -> 512 — with dy read in place from the wider, taller tensor
    whose other values are 3, and the workspace NaN-filled."""
    from lidarnerf import unet_train as ut
    Cin, Cout, H, W, N = R.UPCONV_CASES[k]
    c = T.upconv_backward_case(k)
    x, dcat = _nhwc(c["x"]), _nhwc(c["dcat"])
    outs = []
    for _ in range(2):
        dw, g0 = G.guarded((Cin, Cout, 2, 2), torch.float32)
        db, g1 = G.guarded((Cout,), torch.float32)
        ws, g2 = G.guarded((ut.upconv2x2_backward_weight_workspace_bytes(N, H, W, Cin, Cout) // 4,), torch.float32)
        ut.upconv2x2_backward_weight(x, dcat, ws, dw, db, offset=c["front"])
        assert torch.equal(dw.double(), c["want_dweight"].cuda()), int((dw.double() != c["want_dweight"].cuda()).sum())
        assert torch.equal(db.double(), c["want_dbias"].cuda())
        assert all(G.guard_ok(g) for g in (g0, g1, g2))
        outs.append((dw, db))
    for p, q in zip(*outs):
        assert torch.equal(G._bits(p), G._bits(q))


def test_pool_backward_routes_to_a_nan_as_torch_does():
    """A NaN activation takes the window from any earlier value and keeps it (torch's max-pool); dx itself stays finite."""
    from lidarnerf import unet_train as ut
    c = T.pool_case(0)
    x = c["x"].clone()
    x[0, 1, 0, 1] = x[1, 3, 2, 2] = x[1, 3, 3, 3] = x[0, 5, 5, 7] = float("nan")
    want = T.pool_backward(x, c["dpool"]).permute(0, 2, 3, 1).contiguous().cuda()
    dx, guard = G.guarded(tuple(want.shape), torch.float16)
    ut.pool_backward(_nhwc(x), _nhwc(c["dpool"]), dx)
    assert torch.equal(dx.double(), want) and G.guard_ok(guard) and bool(torch.isfinite(dx).all())
    assert float(dx[0, 0, 1, 1]) == float(c["dpool"][0, 1, 0, 0]) and float(dx[1, 3, 3, 3]) == float(c["dpool"][1, 3, 1, 1])  # (of two NaNs the later one)
