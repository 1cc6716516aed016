"""Host side of the training-mode convolution layer of the ray-drop U-Net (lidarnerf/unet_train.py, csrc/unet_train_conv.hip, the RAW
epilogue of csrc/unet.hip): exports, signatures and every argument refusal of the five entry points and their wrappers,
the workspace sizes against the Python layout, the conditions that make the exact problems of tests/test_unet_train_conv_gpu.py exact,
the pack layouts against torch indexing, the data gradient as a convolution with the flipped and transposed image, and the quantised
restatement of tests/unet_train_conv_cases.py against tests/unet_train_ref.py."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
import unet_train_conv_cases as K
import unet_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1  # LNH_ERR_INVALID_ARG (include/lidarnerf_hip.h)
NEW = ("lnh_unet_pack_conv3x3", "lnh_unet_conv3x3_raw", "lnh_unet_bn_stats", "lnh_unet_bn_stats_workspace_size", "lnh_unet_bn_relu",
       "lnh_unet_bn_relu_backward", "lnh_unet_bn_relu_backward_workspace_size")


def test_exports_and_signatures():
    from lidarnerf import _hip, unet_train
    L = _hip.lib()
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(L, name) and name in text and name in unet_train._SYMBOLS, name
    sigs = _hip._SIGS
    assert len(sigs["lnh_unet_pack_conv3x3"]) == 5 and len(sigs["lnh_unet_conv3x3_raw"]) == len(sigs["lnh_unet_conv3x3"]) - 2
    assert len(sigs["lnh_unet_bn_stats"]) == 15 and sigs["lnh_unet_bn_stats"][5] is C.c_double and sigs["lnh_unet_bn_stats"][6] is C.c_double
    assert len(sigs["lnh_unet_bn_relu"]) == 6 and len(sigs["lnh_unet_bn_relu_backward"]) == 13
    assert L.lnh_unet_bn_stats_workspace_size.restype is C.c_uint64 and L.lnh_unet_bn_relu_backward_workspace_size.restype is C.c_uint64
    for name in ("pack_conv3x3", "conv3x3_raw", "bn_stats", "bn_relu", "bn_relu_backward", "train_workspace_layout", "train_forward",
                 "train_backward"):
        assert callable(getattr(unet_train, name)), name
    assert "ABSENT" in unet_train.train_backward.__doc__


def test_workspace_sizes_are_their_python_twins():
    """The partials are a function of the shape: 256 pixels each up to 2^14 pixels, then 512, ..; never more than 64 of them."""
    from lidarnerf import _hip, unet_train as ut
    L = _hip.lib()
    for M, Cc in ((2, 32), (256, 64), (257, 64), (1020, 1024), (67980, 64), (1 << 14, 32), ((1 << 14) + 1, 32), (1 << 26, 1024)):
        P, parts = ut.bn_partials(M)
        want = parts * 2 * Cc * 8
        assert L.lnh_unet_bn_stats_workspace_size(M, Cc) == L.lnh_unet_bn_relu_backward_workspace_size(M, Cc) == want
        assert ut.bn_stats_workspace_bytes(M, Cc) == ut.bn_relu_backward_workspace_bytes(M, Cc) == want
        assert P % 256 == 0 and (parts - 1) * P < M <= parts * P and parts <= 64
    assert ut.bn_partials(1020) == (256, 4) and ut.bn_partials((1 << 14) + 2) == (512, 33) and ut.bn_partials(67980) == (1280, 54)
    for M, Cc in ((0, 32), (1, 32), ((1 << 26) + 1, 32), (64, 0), (64, 16), (64, 48), (64, 1056)):
        assert L.lnh_unet_bn_stats_workspace_size(M, Cc) == 0 and L.lnh_unet_bn_relu_backward_workspace_size(M, Cc) == 0


def test_train_workspace_layout():
    """The inference layout at its own offsets, then everything training adds: a z and a gradient buffer per layer, the decoder's own
    mid buffers, saved statistics, packed images, parameter gradients, partials workspaces as large as the largest layer needs; every
    buffer 256-byte aligned and none overlapping."""
    from lidarnerf import unet, unet_train as ut
    for N, H, W in ((2, 23, 37), (1, 16, 16), (1, 66, 1030)):
        layout, total = ut.train_workspace_layout(N, H, W)
        names = [e[0] for e in layout]
        assert len(set(names)) == len(names)
        infer, infer_total = unet.workspace_layout(N, H, W)
        assert [(n, o, s) for n, o, s, _ in layout[:len(infer)]] == infer and layout[len(infer)][1] == infer_total
        end = 0
        for name, off, shape, dtype in layout:
            assert off % 256 == 0 and off >= end, name
            n = 1
            for d in shape:
                n *= d
            end = off + n * torch.empty(0, dtype=dtype).element_size()
        assert end <= total < end + 256
        by = {e[0]: e for e in layout}
        sizes = unet.level_sizes(H, W)
        layers = ut.train_layers()
        assert len(layers) == 18 and sum(f"z{k}" in by and f"g{k}" in by and f"stat{k}" in by and f"wf{k}" in by for k in range(18)) == 18
        assert "wb0" not in by and all(f"wb{k}" in by for k in range(1, 18))
        for k, lay in enumerate(layers):
            shape = (N,) + sizes[lay["level"]] + (lay["cout"],)
            assert by[f"z{k}"][2] == by[f"g{k}"][2] == by[lay["out"]][2] == shape and by[f"stat{k}"][2] == (6, lay["cout"])
            assert by[f"wf{k}"][2] == (lay["cout"], 9, max(32, lay["cin"]))
            assert by["ws_bn"][2][0] >= ut.bn_stats_workspace_bytes(shape[0] * shape[1] * shape[2], shape[3])
        assert by["wf0"][2] == (64, 9, 32) and by["wb10"][2] == (1024, 9, 512) and by["dcat0"][2] == (N, H, W, 128)
        assert by["dpool1"][2] == (N, H // 2, W // 2, 64) and by["ws_head"][2][0] == ut.head_backward_workspace_bytes(N, H, W)
        for l in range(4):
            h, w = sizes[l + 1]
            assert by["ws_up"][2][0] >= ut.upconv2x2_backward_weight_workspace_bytes(N, h, w, unet.CHANNELS[l + 1], unet.CHANNELS[l])
    assert {l["out"] for l in ut.train_layers()} == {f"mid{l}" for l in range(5)} | {f"x{l}" for l in range(5)} | \
        {f"dmid{l}" for l in range(4)} | {f"d{l}" for l in range(4)}


def test_every_argument_refusal_of_the_entry_points():
    """Validation happens before any launch, so it runs without a GPU (the pointers are never dereferenced)."""
    from lidarnerf import _hip
    L = _hip.lib()
    p, big = 1 << 20, 1 << 30

    def err():
        return L.lnh_last_error().decode()

    def pack(w=p, Cout=64, Cin=64, fwd=p, bwd=p):
        return L.lnh_unet_pack_conv3x3(w, Cout, Cin, fwd, bwd, None)

    assert pack(w=None) == INVALID_ARG and "null" in err() and pack(fwd=None) == INVALID_ARG and "null" in err()
    for Cout in (0, 32, 96, 1088):
        assert pack(Cout=Cout) == INVALID_ARG and "Cout" in err()
    for Cin in (0, 33, 48, 1056):
        assert pack(Cin=Cin, bwd=None) == INVALID_ARG and "Cin" in err()
    for Cin in (10, 32, 96):
        assert pack(Cin=Cin) == INVALID_ARG and "bwd" in err()
    for kw in (dict(w=p + 4), dict(fwd=p + 2), dict(bwd=p + 8)):
        assert pack(**kw) == INVALID_ARG and "aligned" in err()

    def raw(s0=p, C0=64, H0=17, W0=31, pool=0, s1=None, C1=0, H1=0, W1=0, w=p, N=1, Cout=64, tile=0, out=p):
        return L.lnh_unet_conv3x3_raw(s0, C0, H0, W0, pool, s1, C1, H1, W1, w, N, Cout, tile, out, None)

    for kw in (dict(s0=None), dict(w=None), dict(out=None)):
        assert raw(**kw) == INVALID_ARG and "unet_conv3x3_raw: null" in err()
    assert raw(pool=2) == INVALID_ARG and "pool" in err()
    for C0 in (0, 16, 48, 1056):
        assert raw(C0=C0) == INVALID_ARG and "C0" in err()
    for C1 in (16, 1056):
        assert raw(s1=p, C1=C1, H1=17, W1=31) == INVALID_ARG and "C1" in err()
    assert raw(s1=p) == INVALID_ARG and "together" in err() and raw(C1=64, H1=17, W1=31) == INVALID_ARG and "together" in err()
    for Cout in (0, 32, 96, 1088):
        assert raw(Cout=Cout) == INVALID_ARG and "Cout" in err()
    for kw in (dict(N=0), dict(H0=0), dict(H0=1, pool=1), dict(N=1 << 12, H0=1 << 10, W0=1 << 10)):
        assert raw(**kw) == INVALID_ARG and "source" in err()
    for H1, W1 in ((15, 31), (18, 31), (17, 29), (17, 32), (0, 31)):
        assert raw(s1=p, C1=64, H1=H1, W1=W1) == INVALID_ARG and "second source" in err()
    for kw in (dict(s0=p + 8), dict(w=p + 8), dict(out=p + 8), dict(s1=p + 8, C1=64, H1=17, W1=31)):
        assert raw(**kw) == INVALID_ARG and "aligned" in err()
    for tile in (3, 5, 16):
        assert raw(tile=tile) == INVALID_ARG and "tile" in err()

    def stats(z=p, M=64, Cc=64, gamma=p, beta=p, eps=1e-5, mom=0.1, ws=p, wsb=big, mean=p, invstd=p, scale=p, shift=p, rm=None, rv=None):
        return L.lnh_unet_bn_stats(z, M, Cc, gamma, beta, eps, mom, ws, wsb, mean, invstd, scale, shift, rm, rv, None)

    for k in ("z", "gamma", "beta", "ws", "mean", "invstd", "scale", "shift"):
        assert stats(**{k: None}) == INVALID_ARG and "null" in err(), k
    for M in (0, 1, (1 << 26) + 1):  # one value per channel has no variance: torch refuses it too
        assert stats(M=M) == INVALID_ARG and "M " in err()
    for Cc in (0, 16, 48, 1056):
        assert stats(Cc=Cc) == INVALID_ARG and "C " in err()
    for kw in (dict(eps=-1.0), dict(mom=-0.1), dict(mom=1.5), dict(eps=float("nan"))):
        assert stats(**kw) == INVALID_ARG and "momentum" in err()
    assert stats(M=1020, wsb=4 * 2 * 64 * 8 - 1) == INVALID_ARG and "workspace" in err()
    for k in ("z", "ws", "scale", "shift"):
        assert stats(**{k: p + 8}) == INVALID_ARG and "aligned" in err(), k

    def relu(z=p, M=64, Cc=64, scale=p, shift=p, a=p):
        return L.lnh_unet_bn_relu(z, M, Cc, scale, shift, a, None)

    for k in ("z", "scale", "shift", "a"):
        assert relu(**{k: None}) == INVALID_ARG and "null" in err(), k
        assert relu(**{k: p + 8}) == INVALID_ARG and "aligned" in err(), k
    for M in (0, (1 << 26) + 1):
        assert relu(M=M) == INVALID_ARG and "M " in err()
    for Cc in (0, 16, 48, 1056):
        assert relu(Cc=Cc) == INVALID_ARG and "C " in err()

    def bwd(z=p, a=p, da=p, M=64, Cc=64, mean=p, invstd=p, scale=p, ws=p, wsb=big, dz=p, dgamma=p, dbeta=p):
        return L.lnh_unet_bn_relu_backward(z, a, da, M, Cc, mean, invstd, scale, ws, wsb, dz, dgamma, dbeta, None)

    for k in ("z", "a", "da", "mean", "invstd", "scale", "ws", "dz", "dgamma", "dbeta"):
        assert bwd(**{k: None}) == INVALID_ARG and "null" in err(), k
    for M in (0, 1, (1 << 26) + 1):
        assert bwd(M=M) == INVALID_ARG and "M " in err()
    for Cc in (0, 16, 48, 1056):
        assert bwd(Cc=Cc) == INVALID_ARG and "C " in err()
    assert bwd(M=1020, wsb=4 * 2 * 64 * 8 - 1) == INVALID_ARG and "workspace" in err()
    for k in ("z", "a", "da", "ws", "dz"):
        assert bwd(**{k: p + 8}) == INVALID_ARG and "aligned" in err(), k


def test_wrapper_refusals():
    from lidarnerf import unet, unet_train as ut
    h = torch.zeros(1, 4, 4, 64, dtype=torch.float16)
    v = torch.zeros(64)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.pack_conv3x3(torch.zeros(64, 64, 3, 3), torch.zeros(64, 9, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="GPU"):
        ut.conv3x3_raw(h, torch.zeros(64, 9, 64, dtype=torch.float16), h)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.bn_stats(h, v, v, 1e-5, 0.1, torch.zeros(1 << 12), v, v, v, v)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.bn_relu(h, v, v, h)
    with pytest.raises(RuntimeError, match="GPU"):
        ut.bn_relu_backward(h, h, h, v, v, v, torch.zeros(1 << 12), h, v, v)
    net = unet.RayDropUNet()
    with pytest.raises(ValueError, match="images must be"):
        ut.train_forward(net, torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="at least 16"):
        ut.train_forward(net, torch.zeros(1, 10, 8, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        ut.train_forward(net, torch.zeros(1, 10, 16, 16))
    assert not net.training and int(net.inc.double_conv[1].num_batches_tracked) == 0  # a refused call leaves the module as it was


def test_exact_problems_are_exact():
    """What makes torch.equal the right comparison in tests/test_unet_train_conv_gpu.py.  BatchNorm: every z, a, da, dz is an fp16
    number; each channel has exactly M / 2 of each sign, so mean, variance and their float64 sums have one value; dbeta and dgamma are
    multiples of M and, among the channels, zero and non-zero; the products and sums of the backward are small integers times powers
    of two.  Data gradient: sums of |products| below 2^24.  The values of M cover 2, one partial, several partials with a ragged last
    one, and a pixel count past 2^14 where the partial size doubles; C covers 32 and 96 (a half-used slab of 64 channels), 64, 1024 (16 slabs)."""
    for k, (M, Cc) in enumerate(K.BN_CASES):
        c = K.bn_case(k)
        z, e = c["z"], c["e"]
        assert tuple(z.shape) == (M, Cc) and bool((e.abs() == 1).all()) and not bool(e.sum(0).any())
        for name in ("z", "a", "da", "dz"):
            assert torch.equal(c[name], R.q16(c[name])), (k, name)
        for name in ("mean", "invstd", "scale", "shift", "dbeta", "dgamma", "want_running_mean"):
            assert torch.equal(c[name], R.q32(c[name])), (k, name)
        assert torch.equal(z.mean(0), c["mean"]) and torch.equal((z * z).sum(0) / M - c["mean"] ** 2, c["var"])
        assert torch.equal(c["a"], torch.relu(z * c["scale"] + c["shift"]))
        g = c["da"] * (c["a"] > 0)
        assert torch.equal(g.sum(0), c["dbeta"]) and torch.equal((g * e).sum(0), c["dgamma"])
        assert not bool((c["dbeta"] % M).any()) and not bool((c["dgamma"] % M).any())
        assert bool((c["dgamma"] != 0).any()) and bool((c["dbeta"] != 0).any()) and float(c["da"].abs().max()) <= 16
        assert torch.equal(c["dz"], c["scale"] * (g - c["dbeta"] / M - e * (c["dgamma"] / M)))
        pos, mask = c["z"] > 0, c["a"] > 0  # the wrong mask [z > 0] must show
        assert bool(((pos != mask) & (c["da"] != 0)).any()) or M == 2
        st = K.bn_forward(z.t().reshape(1, Cc, M, 1), c["gamma"], c["beta"], 0.0)  # the restatement gives the same single values
        dz, dgamma, dbeta = K.bn_backward(st, c["da"].t().reshape(1, Cc, M, 1))
        assert torch.equal(st["a"].reshape(Cc, M).t(), c["a"]) and torch.equal(dz.reshape(Cc, M).t(), c["dz"])
        assert torch.equal(dgamma, c["dgamma"]) and torch.equal(dbeta, c["dbeta"]) and torch.equal(st["shift"], c["shift"])
    Ms, Cs = {m for m, _ in K.BN_CASES}, {c for _, c in K.BN_CASES}
    assert Ms >= {2, 64, 66, 4 * 15 * 17} and max(Ms) > 1 << 14 and Cs >= {32, 64, 96, 1024}
    for k in range(len(K.DGRAD_CASES)):
        c = K.dgrad_case(k)
        assert c["bound"] < 2 ** 24 and c["want"].unique().numel() > 20 and bool((c["want"] < 0).any())
        assert torch.equal(c["want"], R.q16(c["want"]))
    assert {(c[0], c[1] + c[2], c[3], c[4]) for c in K.DGRAD_CASES} >= {(64, 64, 15, 17), (128, 128, 16, 16), (1024, 512, 2, 3), (64, 64, 1, 257)}
    assert any(c[5] == 2 for c in K.DGRAD_CASES)
    for index in range(len(R.CONV_CASES)):  # the raw convolution shows what the ReLU epilogue never could: a negative sum
        c = R.conv_case(index)
        raw = F.conv2d(c["x"], c["weight"].double(), padding=1)
        assert bool((raw < 0).any()) and torch.equal(raw, R.q16(raw)) and c["bound"] < 2 ** 24


@pytest.mark.parametrize("k", range(len(K.PACK_CASES)))
def test_pack_layouts_against_torch_indexing(k):
    """fwd is the image lidarnerf.unet packs with torch ops; bwd[ci, t, co] = fp16(W[co, ci, 8 - t])."""
    from lidarnerf import unet
    Cout, Cin = K.PACK_CASES[k]
    w = K.pack_weight(k)
    fwd, bwd = K.pack_images(w)
    conv, bn = torch.nn.Conv2d(Cin, Cout, 3, padding=1, bias=False), torch.nn.BatchNorm2d(Cout)
    with torch.no_grad():
        conv.weight.copy_(w)
    assert torch.equal(fwd, unet.RayDropUNet._pack_conv(conv, bn)[0])
    assert tuple(bwd.shape) == (Cin, 9, Cout)
    for ci, t, co in ((0, 0, 0), (Cin - 1, 8, Cout - 1), (Cin // 2, 5, 3), (1, 2, Cout // 2)):
        assert bwd[ci, t, co] == w[co, ci, (8 - t) // 3, (8 - t) % 3].to(torch.float16)
        assert fwd[co, t, ci] == w[co, ci, t // 3, t % 3].to(torch.float16)
    if Cin < 32:
        assert not bool(fwd[:, :, Cin:].any())


@pytest.mark.parametrize("k", range(len(K.DGRAD_CASES)))
def test_convolution_with_the_bwd_image_is_the_data_gradient(k):
    """conv3x3(dz, bwd) with padding 1 equals F.conv_transpose2d(dz, W, padding=1) in float64, bit for bit on the integer problems."""
    c = K.dgrad_case(k)
    bwd = K.pack_images(c["weight"].float())[1].double()  # [Cin, 9, Cout]
    Cin, _, Cout = bwd.shape
    got = F.conv2d(c["dz"], bwd.reshape(Cin, 3, 3, Cout).permute(0, 3, 1, 2), padding=1)
    assert torch.equal(got, c["want"])
    wrong = c["weight"].flip(2, 3).permute(1, 0, 2, 3)  # (and is not symmetric: without the flip it differs)
    assert not torch.equal(F.conv2d(c["dz"], c["weight"].permute(1, 0, 2, 3), padding=1), c["want"]) and \
        torch.equal(F.conv2d(c["dz"], wrong, padding=1), c["want"])


def test_restatement_without_quantisation_is_the_float64_reference():
    sd, x, cot = R.hash_state_dict(), T.g18_train_batch(), T.g18_train_cotangent()
    want_logits, want_state = T.unet_train_forward(sd, x)
    want = T.unet_backward_from_state(sd, want_state, cot)
    logits, state = K.unet_train_forward(sd, x, quantize=False)
    grads = K.unet_train_backward(sd, state, cot, quantize=False)
    assert float((logits - want_logits).abs().max()) <= 1e-10
    assert len(K.GRAD_NAMES) == 46 and set(grads) == set(K.GRAD_NAMES)
    for name in K.GRAD_NAMES:
        assert float((grads[name] - want[name]).norm()) <= 1e-10 * float(want[name].norm()), name
    # with it on: one layer's z, a are fp16 numbers, the saved vectors f32 numbers, and the logits stay near the reference
    logits_q, state_q = K.unet_train_forward(sd, x, quantize=True)
    st = state_q["layers"][5]
    assert torch.equal(st["z"], R.q16(st["z"])) and torch.equal(st["a"], R.q16(st["a"])) and torch.equal(st["s"], R.q32(st["s"]))
    assert 0 < float((logits_q - want_logits).abs().max()) < 0.1
