"""Host side of the ray-drop U-Net (csrc/unet.hip, lidarnerf/unet.py): exports and signatures, every refusal, the workspace size,
state-dict names and shapes against the reference's (golden G17), round trips through stock torch modules, the float64
restatement (tests/unet_ref.py) against G17's tensors, the packing layout, and the conditions that make the exact known-answer
tests of tests/test_unet_gpu.py meaningful."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import unet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID_ARG = -1  # LNH_ERR_INVALID_ARG (include/lidarnerf_hip.h)
NAMES = ("lnh_unet_input", "lnh_unet_conv3x3", "lnh_unet_upconv2x2", "lnh_unet_head")


def _g17(name="g17_unet"):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


_SD = {}


def _hash_sd():
    if "sd" not in _SD:
        _SD["sd"] = R.hash_state_dict()
    return _SD["sd"]


def test_exports_and_signatures():
    from lidarnerf import _hip
    L = _hip.lib()
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    for name in NAMES + ("lnh_unet_workspace_size",):
        assert name in _hip.EXPORTS and hasattr(L, name) and name in text, name
    assert [len(_hip._SIGS[n]) for n in NAMES] == [6, 16, 9, 8]
    assert L.lnh_unet_workspace_size.restype is C.c_uint64
    assert (_hip.UNET_TILE_16, _hip.UNET_TILE_32, _hip.UNET_TILE_64, _hip.UNET_TILE_KSPLIT) == (1, 2, 4, 8)
    for k, v in (("LNH_UNET_TILE_16", 1), ("LNH_UNET_TILE_32", 2), ("LNH_UNET_TILE_64", 4), ("LNH_UNET_TILE_KSPLIT", 8)):
        assert f"#define {k} {v}u" in text


def test_workspace_size_is_the_layout():
    from lidarnerf import _hip, unet
    L = _hip.lib()
    for N, H, W in ((1, 16, 16), (2, 23, 37), (1, 66, 1030), (3, 17, 16)):
        layout, total = unet.workspace_layout(N, H, W)
        assert L.lnh_unet_workspace_size(N, H, W) == total > 0
        assert [n for n, _, _ in layout] == ["input"] + [f"{a}{l}" for l in range(5) for a in ("mid", "x")] + \
            [f"{a}{l}" for l in range(4) for a in ("up", "d")]
        end = 0
        for name, off, shape in layout:  # aligned, in order, not overlapping
            assert off % 256 == 0 and off >= end
            end = off + int(np.prod(shape)) * 2
        assert end <= total
        shapes = {n: s for n, _, s in layout}
        assert shapes["input"] == (N, H, W, 32) and shapes["x4"] == (N, H >> 4, W >> 4, 1024)
        assert shapes["up0"] == (N, 2 * (H >> 1), 2 * (W >> 1), 64) and shapes["d0"] == (N, H, W, 64)
    assert unet.workspace_layout(1, 66, 1030)[1] < 100 << 20
    for N, H, W in ((0, 16, 16), (1, 15, 16), (1, 16, 15), (1, 8192, 8193), (65, 1024, 1024)):
        assert L.lnh_unet_workspace_size(N, H, W) == 0


def test_every_argument_refusal_of_the_entry_points():
    """Validation happens before any launch, so it runs without a GPU (the pointers are never dereferenced)."""
    from lidarnerf import _hip
    L = _hip.lib()
    p = 1 << 20

    def err():
        return L.lnh_last_error().decode()

    def conv(src0=p, C0=64, H0=17, W0=19, pool=0, src1=None, C1=0, H1=0, W1=0, w=p, s=p, t=p, N=1, Cout=64, tile=0, out=p):
        return L.lnh_unet_conv3x3(src0, C0, H0, W0, pool, src1, C1, H1, W1, w, s, t, N, Cout, tile, out, None)

    for kw in (dict(src0=None), dict(w=None), dict(s=None), dict(t=None), dict(out=None)):
        assert conv(**kw) == INVALID_ARG and "null" in err()
    for C0 in (0, 10, 48, 1056):
        assert conv(C0=C0) == INVALID_ARG and "C0" in err()
    for C1 in (16, 1056):
        assert conv(src1=p, C1=C1, H1=17, W1=19) == INVALID_ARG and "C1" in err()
    assert conv(src1=p, C1=0) == INVALID_ARG and "together" in err()
    assert conv(src1=None, C1=64, H1=17, W1=19) == INVALID_ARG and "together" in err()
    for Cout in (0, 32, 96, 1088):
        assert conv(Cout=Cout) == INVALID_ARG and "Cout" in err()
    assert conv(pool=2) == INVALID_ARG and "pool" in err()
    assert conv(N=0) == INVALID_ARG and conv(H0=0) == INVALID_ARG and conv(H0=1, W0=19, pool=1) == INVALID_ARG
    assert conv(N=1 << 12, H0=1 << 10, W0=1 << 10) == INVALID_ARG and "2^26" in err()
    for H1, W1 in ((15, 19), (17, 17), (18, 19), (17, 20), (0, 19)):
        assert conv(src1=p, C1=64, H1=H1, W1=W1) == INVALID_ARG and "second source" in err()
    for kw in (dict(src0=p + 8), dict(w=p + 2), dict(s=p + 4), dict(t=p + 4), dict(out=p + 8), dict(src1=p + 8, C1=64, H1=17, W1=19)):
        assert conv(**kw) == INVALID_ARG and "aligned" in err()
    for tile in (3, 5, 16):
        assert conv(tile=tile) == INVALID_ARG and "tile" in err()

    assert L.lnh_unet_input(None, 1, 10, 16, 16, p, None) == INVALID_ARG and "null" in err()
    assert L.lnh_unet_input(p, 1, 10, 16, 16, None, None) == INVALID_ARG
    for Cc in (0, 33):
        assert L.lnh_unet_input(p, 1, Cc, 16, 16, p, None) == INVALID_ARG and "channels" in err()
    assert L.lnh_unet_input(p, 0, 10, 16, 16, p, None) == INVALID_ARG and L.lnh_unet_input(p, 1, 10, 16, 16, p + 8, None) == INVALID_ARG

    def up(x=p, N=1, H=4, W=5, Cin=128, w=p, b=p, Cout=64, out=p):
        return L.lnh_unet_upconv2x2(x, N, H, W, Cin, w, b, Cout, out, None)

    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(out=None)):
        assert up(**kw) == INVALID_ARG and "null" in err()
    for Cin in (0, 16, 1056):
        assert up(Cin=Cin) == INVALID_ARG and "Cin" in err()
    for Cout in (0, 32, 1088):
        assert up(Cout=Cout) == INVALID_ARG and "Cout" in err()
    assert up(N=0) == INVALID_ARG and up(N=1 << 10, H=1 << 10, W=1 << 5) == INVALID_ARG
    assert up(x=p + 8) == INVALID_ARG and "aligned" in err()

    assert L.lnh_unet_head(None, 1, 16, 16, p, p, p, None, None) == INVALID_ARG and "null" in err()
    assert L.lnh_unet_head(p, 1, 16, 16, p, None, p, None, None) == INVALID_ARG
    assert L.lnh_unet_head(p, 1, 16, 16, p, p, None, None, None) == INVALID_ARG
    assert L.lnh_unet_head(p, 0, 16, 16, p, p, p, None, None) == INVALID_ARG
    assert L.lnh_unet_head(p + 8, 1, 16, 16, p, p, p, None, None) == INVALID_ARG and "aligned" in err()


def test_module_refusals():
    from lidarnerf.unet import RayDropUNet
    with pytest.raises(NotImplementedError, match="bilinear"):
        RayDropUNet(bilinear=True)
    with pytest.raises(NotImplementedError, match="n_classes"):
        RayDropUNet(n_classes=2)
    with pytest.raises(ValueError, match="n_channels"):
        RayDropUNet(n_channels=33)
    net = RayDropUNet()
    assert not net.training and (net.n_channels, net.n_classes, net.bilinear) == (10, 1, False)
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(1, 10, 16, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        net.predict_mask(torch.zeros(1, 10, 16, 16))
    for shape in ((1, 10, 15, 16), (1, 10, 16, 15)):
        with pytest.raises(ValueError, match="at least 16"):
            net(torch.zeros(shape))
    for shape in ((1, 9, 16, 16), (10, 16, 16)):
        with pytest.raises(ValueError, match="images must be"):
            net(torch.zeros(shape))
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):
        net(torch.zeros(1, 10, 16, 16))


def test_state_dict_is_the_references():
    from lidarnerf.unet import RayDropUNet
    g = _g17()
    want = [(str(n), tuple(int(v) for v in str(s).split(",") if v)) for n, s in zip(g["names"], g["shapes"])]
    assert len(want) == 18 * 6 + 8 + 2 and want == R.state_spec(10)
    net = RayDropUNet()
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    assert net.state_dict()["inc.double_conv.1.num_batches_tracked"].dtype == torch.int64
    assert sum(v.numel() for v in net.parameters()) == 31037633 + 7 * 64 * 9  # (the 3-channel net of the literature, plus 7 input channels)


def test_round_trip_through_stock_modules(tmp_path):
    """The hashed state dict into RayDropUNet, its state_dict() into the same net of stock torch modules (strict), a checkpoint file
    back through from_checkpoint's path; and the stock net, in float64, computes what the restatement computes — so the names carry
    the roles the restatement gives them."""
    from lidarnerf.unet import RayDropUNet
    sd = _hash_sd()
    net = RayDropUNet()
    net.load_state_dict(sd)
    stock = R.stock_unet()
    stock.load_state_dict(net.state_dict(), strict=True)
    for k, v in stock.state_dict().items():
        assert torch.equal(v, sd[k]), k
    path = os.path.join(tmp_path, "ckpt.pth")
    torch.save(stock.state_dict(), path)
    again = RayDropUNet()
    again.load_state_dict(torch.load(path, map_location="cpu"))
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k]), k
    x = R.g17_image(0)
    with torch.no_grad():
        got = stock.double().eval()(x.double())
    assert float((got - R.unet_forward(sd, x)).abs().max()) < 1e-10


def test_restatement_equals_the_reference():
    g, frame = _g17(), _g17("g17_unet_frame")
    sd = _hash_sd()
    for name in R.G17_BLOCKS:
        got = R.block_forward(name, sd, R.g17_block_inputs(name))
        want = torch.from_numpy(g[f"block_{name}"])
        assert got.shape == want.shape and float((got - want).abs().max()) < 1e-10, name
        assert 0 < float(g[f"dev_amp16_block_{name}"]) < 0.1
    assert g["block_up"].shape == (1, 64, 17, 19) and g["block_down"].shape == (1, 128, 8, 9)
    for i, want in enumerate((g["logits64_0"], frame["logits64_1"])):
        got = R.unet_forward(sd, R.g17_image(i))
        assert got.shape == (1, 1) + R.G17_SIZES[i] and float((got - torch.from_numpy(want)).abs().max()) < 1e-10
        assert float(g[f"left_out_{i}"]) < 0.05 and float(g[f"dev_amp16_{i}"]) < 0.02 * float(g[f"std_{i}"])


def test_quantized_restatement_is_what_the_fixture_recorded():
    g, quant = _g17(), _g17("g17_unet_quant")
    sd = _hash_sd()
    q = R.unet_forward(sd, R.g17_image(0), quantize=True)
    assert torch.equal(q.float(), torch.from_numpy(quant["quant_0"]))
    assert float((q - torch.from_numpy(g["logits64_0"])).abs().max()) == float(g["dev_quant_0"]) < float(g["dev_amp16_0"])
    assert quant["quant_1"].shape == (1, 1, 66, 1030) and float(g["dev_quant_1"]) < float(g["dev_amp16_1"])


def test_packing_layout():
    from lidarnerf.unet import RayDropUNet
    sd = _hash_sd()
    net = RayDropUNet()
    net.load_state_dict(sd)  # (packs)
    packed = net._packed
    assert len(packed["convs"]) == 18 and len(packed["ups"]) == 4
    prefixes = ["inc.double_conv"] + [f"down{i}.maxpool_conv.1.double_conv" for i in range(1, 5)] + \
        [f"up{i}.conv.double_conv" for i in range(1, 5)]
    k = 0
    for prefix in prefixes:
        for conv, bn in (("0", "1"), ("3", "4")):
            img, s, t = packed["convs"][k]
            k += 1
            w = sd[f"{prefix}.{conv}.weight"]
            cout, cin = w.shape[:2]
            cpad = (cin + 31) // 32 * 32
            assert img.dtype == torch.float16 and tuple(img.shape) == (cout, 9, cpad) and img.is_contiguous()
            for ky, kx, co, ci in ((0, 0, 0, 0), (1, 2, cout - 1, cin - 1), (2, 1, 5, 3)):
                assert img[co, 3 * ky + kx, ci] == w[co, ci, ky, kx].to(torch.float16)
            assert torch.equal(img[:, :, :cin], w.permute(0, 2, 3, 1).reshape(cout, 9, cin).to(torch.float16))
            assert not bool(img[:, :, cin:].any())
            s64, t64 = R.bn_scale_shift(*[sd[f"{prefix}.{bn}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")])
            assert s.dtype == torch.float32 and torch.equal(s, s64.float()) and torch.equal(t, t64.float())
    assert packed["convs"][0][0].shape == (64, 9, 32)
    for i in range(4):
        img, b = packed["ups"][i]
        w = sd[f"up{i + 1}.up.weight"]
        assert img.dtype == torch.float16 and tuple(img.shape) == (4, w.shape[1], w.shape[0])
        for dy, dx, co, ci in ((0, 0, 0, 0), (1, 0, 7, 9), (0, 1, w.shape[1] - 1, w.shape[0] - 1), (1, 1, 3, 2)):
            assert img[2 * dy + dx, co, ci] == w[ci, co, dy, dx].to(torch.float16)
        assert torch.equal(b, sd[f"up{i + 1}.up.bias"])
    hw, hb = packed["head"]
    assert torch.equal(hw, sd["outc.conv.weight"].reshape(64).to(torch.float16)) and torch.equal(hb, sd["outc.conv.bias"])
    with torch.no_grad():  # a changed parameter is picked up by pack()
        net.outc.conv.bias.fill_(1.5)
    assert float(net.pack()["head"][1]) == 1.5


def test_integer_problems_are_exact():
    """What makes torch.equal the right comparison in tests/test_unet_gpu.py: the quantised restatement (fp16 weights and
    activations, fp32 epilogue) equals the float64 one, so no rounding happens anywhere, and every sum of |products| stays below
    2^24, so fp32 accumulation is exact in any order."""
    assert len(R.CONV_CASES) == 18
    seen = set()
    for i, (C0, C1, Cout, H, W, pool, off, N) in enumerate(R.CONV_CASES):
        c = R.conv_case(i)
        assert c["bound"] < 2 ** 24 and c["want"].shape == (N, Cout, H, W)
        assert torch.equal(c["want"], R.conv_scale_shift_relu(R.q16(c["x"]), c["weight"], c["scale"], c["shift"], quantize=True))
        assert torch.equal(c["weight"], c["weight"].to(torch.float16).float()) and float(c["weight"].abs().max()) == 2
        assert 0.2 < float((c["want"] > 0).double().mean()) < 0.8 and c["want"].unique().numel() > 40
        assert set(c["scale"].tolist()) == {0.25, 0.5, 1.0, 2.0}
        seen.add((C0, C1, Cout))
        if pool:
            assert c["src0"].shape[2] == 2 * H + 1 and c["src0"].shape[3] in (2 * W, 2 * W + 1)
    assert {(10, 0, 64), (64, 0, 128), (64, 64, 64), (512, 512, 512)} <= seen
    assert {c[6] for c in R.CONV_CASES if c[1]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for i in range(len(R.UPCONV_CASES)):
        c = R.upconv_case(i)
        assert c["bound"] < 2 ** 24 and torch.equal(c["want"], R.upconv(c["x"].double(), c["weight"], c["bias"], quantize=True))
        assert c["want"].unique().numel() > 20
    h = R.head_case()
    assert float(h["want"][0, 0, 0, 0]) == 0.0 and bool(torch.isnan(h["want"][0, 0, 0, 1])) and h["want"][0, 0, 0, 2] != 0
    finite = ~torch.isnan(h["want"])
    assert torch.equal(h["want"][finite], R.head(R.q16(h["x"].double()), h["weight"], h["bias"], quantize=True)[finite])
    sd = R.integer_state_dict()
    for H, W in ((16, 16), (23, 37)):
        x = R.integer_image(2900, (1, 10, H, W))
        a, b = R.integer_unet_forward(sd, x), R.integer_unet_forward(sd, x, quantize=True)
        assert torch.equal(a, b) and float(a.abs().max()) < 2 ** 24
        assert a.unique().numel() > 100 and float((a != 0).double().mean()) > 0.5  # the net is alive


def test_host_answers_are_as_recorded():
    """Every lnh_unet_* entry point with each argument it refuses (and calls wrong in two ways, which pin the order of the checks):
    return code and lnh_last_error() text; every *_workspace_size function on the levels of the shapes the layout tests use and on
    what it answers 0 for — the table of tests/unet_host_cases.py against tests/golden/unet_host.json, recorded from the library
    of the commit named in that file.  No call reaches a launch: the record holds a refusal for each one, which is asserted before
    anything is called."""
    import json

    import unet_host_cases as cases
    from lidarnerf import _hip
    with open(os.path.join(GOLDEN, "unet_host.json")) as f:
        rec = json.load(f)
    lib = _hip.lib()
    assert lib.lnh_version() == rec["recorded_from"]["lnh_version"]
    want = rec["refusals"]
    names = [name for name, _, _ in cases.calls()]
    assert set(names) == set(want) and len(names) == len(set(names)) >= 400
    assert all(a["rc"] == INVALID_ARG == cases.INVALID_ARG and a["error"] for a in want.values())
    unet_exports = {n for n in _hip.EXPORTS if n.startswith("lnh_unet_")}
    assert {n for n in unet_exports if not n.endswith("_workspace_size")} == set(cases.BASES) == set(cases.WRONG)
    assert all(sum("+" in case for case in cases.WRONG[fn]) >= 2 for fn in cases.WRONG)
    got = cases.refusal_answers(lib, only=set(want))
    for name in sorted(want):
        assert got[name] == want[name], (name, got[name], want[name])
    sizes = rec["sizes"]
    assert {fn for _, fn, _ in cases.size_calls()} == {n for n in unet_exports if n.endswith("_workspace_size")}
    got = cases.size_answers(lib)
    assert set(got) == set(sizes)
    for name in sorted(sizes):
        assert got[name] == sizes[name], (name, got[name], sizes[name])
    # the record itself holds what it is meant to pin: nothing but the listed shapes answers 0, and no size function touches the error
    for name, a in sizes.items():
        dead = "/zero/" in name or ("/1x16x16/" in name and name.startswith("lnh_unet_bn_") and name.endswith(("layer8", "layer9")))
        assert (a["bytes"] == 0) == dead, name
    assert len({a["error"] for a in sizes.values()}) == 1
