"""Host side of the 3 x 3 convolution's weight gradient and of the full backward of the ray-drop U-Net (csrc/unet_train_wgrad.hip,
lidarnerf/unet_train.py): exports and signatures, the workspace size against its Python twin and the split rule, every
argument refusal (validation happens before any launch, so none needs a GPU), the workspace layout's new buffers, and the conditions
that make the problems of tests/test_unet_train_step_gpu.py exact."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import unet_train_wgrad_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1  # LNH_ERR_INVALID_ARG (include/lidarnerf_hip.h)
NEW = ("lnh_unet_conv3x3_backward_weight", "lnh_unet_conv3x3_backward_weight_workspace_size")


def test_exports_and_signatures():
    from lidarnerf import _hip, unet_train
    L = _hip.lib()
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    for name in NEW:
        assert name in _hip.EXPORTS and hasattr(L, name) and name in text and name in unet_train._SYMBOLS, name
    sig = _hip._SIGS["lnh_unet_conv3x3_backward_weight"]
    assert len(sig) == 17 and sig[15] is C.c_uint64
    assert L.lnh_unet_conv3x3_backward_weight_workspace_size.restype is C.c_uint64
    assert (_hip.UNET_WGRAD_GATHER, _hip.UNET_WGRAD_TR) == (1, 2)
    assert "LNH_UNET_WGRAD_GATHER 1u" in text and "LNH_UNET_WGRAD_TR 2u" in text
    for name in ("conv3x3_backward_weight", "conv3x3_backward_weight_workspace_bytes", "conv_wgrad_slices"):
        assert callable(getattr(unet_train, name)), name
    doc = unet_train.train_backward.__doc__
    assert "ABSENT" in doc and "conv_weights" in doc


def test_workspace_size_is_its_python_twin_and_the_split_is_a_function_of_the_shape():
    """S = min(ceil(M / 256), max(1, 32 MiB / (36 Cp Cout))) slices of ceil(M / S) pixels rounded up to 32; S x 36 Cp Cout bytes.  The
    layers of a 66 x 1030 frame: 266 slices for the first, one partial copy for everything of 256 x 512 channels and more."""
    from lidarnerf import _hip, unet_train as ut
    L = _hip.lib()
    size = L.lnh_unet_conv3x3_backward_weight_workspace_size
    for N, H0, W0, pool, C0, C1, Cout in ((1, 16, 16, 0, 32, 0, 64), (2, 17, 31, 0, 32, 0, 64), (2, 35, 67, 1, 64, 0, 128),
                                          (1, 1, 257, 0, 64, 0, 64), (1, 17, 31, 0, 64, 64, 64), (1, 4, 6, 0, 512, 512, 512),
                                          (2, 2, 3, 0, 1024, 0, 1024), (1, 66, 1030, 0, 32, 0, 64), (1, 66, 1030, 0, 64, 64, 64),
                                          (1, 8, 128, 1, 512, 0, 1024), (1, 8, 128, 0, 512, 512, 512), (1, 1 << 13, 1 << 13, 0, 64, 0, 64)):
        H, W = (H0 // 2, W0 // 2) if pool else (H0, W0)
        M, Cp = N * H * W, C0 + C1
        S, Lp = ut.conv_wgrad_slices(M, Cp, Cout)
        want = S * 36 * Cp * Cout
        assert size(N, H0, W0, pool, C0, C1, Cout) == ut.conv3x3_backward_weight_workspace_bytes(N, H0, W0, pool, C0, C1, Cout) == want
        assert Lp % 32 == 0 and (S - 1) * Lp < M <= S * Lp and (S == 1 or want <= 32 << 20)
    assert ut.conv_wgrad_slices(256, 32, 64) == (1, 256) and ut.conv_wgrad_slices(1054, 32, 64) == (5, 224)
    assert ut.conv_wgrad_slices(24, 1024, 512) == (1, 32) and ut.conv_wgrad_slices(12, 1024, 1024) == (1, 32)
    assert ut.conv_wgrad_slices(67980, 32, 64) == (266, 256) and ut.conv_wgrad_slices(1024, 1024, 512) == (1, 1024)
    assert ut.conv_wgrad_slices(256, 1024, 1024) == (1, 256) and 36 * 1024 * 1024 == 37748736  # the deepest layer: one partial copy
    # the finishing kernel changes at more than 8 slices: the exact problems cover both sides of that threshold
    slices = {i: ut.conv_wgrad_slices(c[7] * c[3] * c[4], max(32, c[0]) + c[1], c[2])[0] for i, c in zip(WC.WGRAD_IDS, WC.WGRAD_CASES)}
    assert slices["h"] == 10 and slices["b"] == 5 and slices["a"] == slices["f"] == slices["g"] == 1
    assert max(v for k, v in slices.items() if k != "h") <= 8
    refused = ((0, 16, 16, 0, 64, 0, 64), (1, 0, 16, 0, 64, 0, 64), (1, 1, 16, 1, 64, 0, 64), (1, 16, 16, 2, 64, 0, 64),
               (1 << 12, 1 << 10, 1 << 10, 0, 64, 0, 64), (1, 16, 16, 0, 0, 0, 64), (1, 16, 16, 0, 16, 0, 64), (1, 16, 16, 0, 96, 0, 64),
               (1, 16, 16, 0, 1088, 0, 64), (1, 16, 16, 0, 32, 32, 64), (1, 16, 16, 0, 128, 64, 64), (1, 16, 16, 0, 64, 128, 64),
               (1, 16, 16, 0, 64, 0, 0), (1, 16, 16, 0, 64, 0, 32), (1, 16, 16, 0, 64, 0, 96), (1, 16, 16, 0, 64, 0, 1088))
    for args in refused:
        assert size(*args) == 0 and ut.conv3x3_backward_weight_workspace_bytes(*args) == 0, args


def test_every_argument_refusal():
    """Each unsupported channel combination, a workspace one byte short, a pointer that is not 16-byte aligned, a second source of the
    wrong size: refused with a message before anything is launched (the pointers are never dereferenced)."""
    from lidarnerf import _hip
    L = _hip.lib()
    p, big = 1 << 20, 1 << 40

    def err():
        return L.lnh_last_error().decode()

    def wgrad(s0=p, C0=64, H0=17, W0=31, pool=0, s1=None, C1=0, H1=0, W1=0, dz=p, N=1, Cout=64, Cin=None, variant=0, ws=p, wsb=big,
              dw=p):
        Cin = C0 + C1 if Cin is None else Cin
        return L.lnh_unet_conv3x3_backward_weight(s0, C0, H0, W0, pool, s1, C1, H1, W1, dz, N, Cout, Cin, variant, ws, wsb, dw, None)

    for k in ("s0", "dz", "ws", "dw"):
        assert wgrad(**{k: None}) == INVALID_ARG and "unet_conv3x3_backward_weight: null" in err(), k
    assert wgrad(pool=2) == INVALID_ARG and "pool" in err()
    for C0 in (0, 16, 48, 96, 1088):
        assert wgrad(C0=C0) == INVALID_ARG and "C0" in err(), C0
    for C0, C1 in ((64, 32), (64, 128), (128, 64), (32, 32), (1024, 512)):
        assert wgrad(C0=C0, s1=p, C1=C1, H1=17, W1=31) == INVALID_ARG and "C1" in err(), (C0, C1)
    assert wgrad(s1=p) == INVALID_ARG and "together" in err() and wgrad(C1=64, H1=17, W1=31) == INVALID_ARG and "together" in err()
    for Cout in (0, 32, 96, 1088):
        assert wgrad(Cout=Cout) == INVALID_ARG and "Cout" in err()
    for C0, Cin in ((64, 10), (64, 63), (64, 128), (32, 0), (32, 33)):
        assert wgrad(C0=C0, Cin=Cin) == INVALID_ARG and "Cin" in err(), (C0, Cin)
    for kw in (dict(N=0), dict(H0=0), dict(H0=1, pool=1), dict(N=1 << 12, H0=1 << 10, W0=1 << 10)):
        assert wgrad(**kw) == INVALID_ARG and "source" in err()
    for H1, W1 in ((15, 31), (18, 31), (17, 29), (17, 32), (0, 31)):
        assert wgrad(s1=p, C1=64, H1=H1, W1=W1) == INVALID_ARG and "second source" in err()
    for variant in (3, 4, 8):
        assert wgrad(variant=variant) == INVALID_ARG and "variant" in err()
    need = L.lnh_unet_conv3x3_backward_weight_workspace_size(1, 17, 31, 0, 64, 0, 64)
    assert need == 3 * 36 * 64 * 64 and wgrad(wsb=need - 1) == INVALID_ARG and "workspace" in err()
    for kw in (dict(s0=p + 8), dict(dz=p + 8), dict(ws=p + 8), dict(dw=p + 4), dict(s1=p + 8, C1=64, H1=17, W1=31)):
        assert wgrad(**kw) == INVALID_ARG and "aligned" in err(), kw


def test_train_workspace_layout_appends_the_weight_gradients():
    """dcw{k} f32 in the parameter's shape and ws_cw follow everything that was there, 256-byte aligned; ws_cw holds the largest layer's
    partials; the state-dict names of the 64 gradients are the net's parameters."""
    import unet_ref as R
    from lidarnerf import unet, unet_train as ut
    spec = dict(R.state_spec())
    for N, H, W in ((2, 23, 37), (1, 66, 1030)):
        layout, total = ut.train_workspace_layout(N, H, W)
        names = [e[0] for e in layout]
        first = names.index("dcw0")
        assert names[first - 1] == "logits" and names[first:] == [f"dcw{k}" for k in range(18)] + ["ws_cw"]
        by = {e[0]: e for e in layout}
        sizes = unet.level_sizes(H, W)
        for k, lay in enumerate(ut.train_layers()):
            name, off, shape, dtype = by[f"dcw{k}"]
            assert off % 256 == 0 and dtype == torch.float32 and shape == tuple(spec[lay["conv"] + ".weight"]) == (lay["cout"], lay["cin"], 3, 3)
            h0, w0 = sizes[lay["level"] - 1] if lay["pool"] else sizes[lay["level"]]
            c0, c1 = (lay["cin"] // 2, lay["cin"] // 2) if lay["src1"] else (max(32, lay["cin"]), 0)
            need = ut.conv3x3_backward_weight_workspace_bytes(N, h0, w0, lay["pool"], c0, c1, lay["cout"])
            assert 0 < need <= by["ws_cw"][2][0]
        assert by["ws_cw"][1] % 256 == 0 and by["ws_cw"][1] + by["ws_cw"][2][0] <= total
        assert by["ws_cw"][2][0] == 36 * 1024 * 1024


@pytest.mark.parametrize("k", range(len(WC.WGRAD_CASES)), ids=WC.WGRAD_IDS)
def test_the_integer_problems_are_exact(k):
    """Every sum of |products| below 2^24 (so every partial and total is an integer fp32 holds), operands fp16-valued, the answer not
    trivial; the float64 answer is the gradient autograd gives for the convolution of the concatenated, pooled, padded operand."""
    c = WC.wgrad_case(k)
    C0, C1, Cout, H, W, src, off, N = WC.WGRAD_CASES[k]
    assert c["bound"] < 2 ** 24 and c["want"].shape == (Cout, C0 + C1, 3, 3) and c["want"].dtype == torch.float64
    assert torch.equal(c["want"], c["want"].round()) and c["want"].unique().numel() >= 8
    for t in (c["src0"], c["dz"]) + (() if c["src1"] is None else (c["src1"],)):
        assert torch.equal(t, t.half().float())
    assert 0.15 < float((c["dz"] != 0).float().mean()) < 0.35 and float(c["dz"].abs().max()) == 2 and float(c["src0"].max()) == 3
    if k in (0, 2, 4, 8):  # autograd of the convolution itself, on the cheap cases
        w = torch.zeros(Cout, C0 + C1, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(c["x"], w, padding=1).backward(c["dz"].double())
        assert torch.equal(w.grad, c["want"])
    if WC.WGRAD_IDS[k] == "d":
        assert not c["want"][:, :, 0].any() and not c["want"][:, :, 2].any() and c["want"][:, :, 1].any()
    if WC.WGRAD_IDS[k] in ("c", "c2"):  # a source row / column that no window covers holds values that would change the answer
        assert src[0] % 2 == 1 and float(c["src0"][:, :, -1].max()) == 3
    if off is not None and off != (0, 0):  # the padded row / column of the second source contributes nothing
        xs = c["x"][:, C0:]
        assert (off[0] == 0 or not xs[:, :, -1].any()) and (off[1] == 0 or not xs[:, :, :, -1].any())
