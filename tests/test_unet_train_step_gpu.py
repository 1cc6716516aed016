"""The 3 x 3 convolution's weight gradient on the device (csrc/unet_train_wgrad.hip) and train_backward with all 64 gradients
(lidarnerf/unet_train.py), in the habits of tests/test_unet_train_conv_gpu.py: every output NaN-filled before the call and followed by
guard words, every call made twice with equal bits, torch.equal wherever the problem has one answer
(tests/test_unet_train_step_cpu.py asserts the conditions).  The one bound used comes from the stock net's own fp16-autocast run on the
CPU, never from the device, and the test prints its figures before it asserts."""
import functools

import pytest
import torch

import test_unet_gpu as G
import test_unet_train_conv_gpu as TC
import unet_ref as R
import unet_train_conv_cases as K
import unet_train_ref as T
import unet_train_wgrad_cases as WC

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 2)  # the default, 16-bit LDS gathers, transposed LDS reads: one answer, one set of bits


def _operands(c):
    src0 = G.nhwc16(c["src0"])
    src1 = None if c["src1"] is None else G.nhwc16(c["src1"])
    return src0, src1, G.nhwc16(c["dz"])


def _run(c, src0, src1, dz, cin, variant=0, ws_fill=float("nan")):
    """One guarded call: (dweight, bits ok) with the workspace of exactly the size the twin states, NaN-filled."""
    from lidarnerf import unet_train as ut
    N, H0, W0, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    Cout = dz.shape[3]
    need = ut.conv3x3_backward_weight_workspace_bytes(N, H0, W0, c["pool"], C0, C1, Cout)
    assert need > 0 and need % 4 == 0
    ws, gw = G.guarded((need // 4,), torch.float32)
    ws.fill_(ws_fill)
    dw, gd = G.guarded((Cout, cin, 3, 3), torch.float32)
    ut.conv3x3_backward_weight(src0, dz, ws, dw, src1=src1, pool=c["pool"], variant=variant)
    torch.cuda.synchronize()
    assert G.guard_ok(gw) and G.guard_ok(gd)
    return dw


@pytest.mark.parametrize("k", range(len(WC.WGRAD_CASES)), ids=WC.WGRAD_IDS)
def test_weight_gradient_exact(k):
    """The twelve integer problems of unet_train_wgrad_cases against the float64 gradient of F.conv2d on the concatenated, pooled,
    padded operand: every variant, every call twice, the same bits throughout; the padded first layer writes 10 channels of its 32
    and nothing behind them; at 1 x 257 six of the nine planes are exactly zero."""
    c = WC.wgrad_case(k)
    cin = WC.WGRAD_CASES[k][0] + WC.WGRAD_CASES[k][1]
    src0, src1, dz = _operands(c)
    assert src0.shape[3] == max(32, WC.WGRAD_CASES[k][0])
    want = c["want"].cuda()
    first = None
    for variant in VARIANTS:
        for _ in range(2):
            dw = _run(c, src0, src1, dz, cin, variant)
            bad = dw.double() != want
            assert not bool(bad.any()), (variant, int(bad.sum()), bad.nonzero()[:4].tolist())
            first = dw if first is None else first
            assert torch.equal(G._bits(dw), G._bits(first)), variant
    if WC.WGRAD_IDS[k] == "d":
        assert not bool(first[:, :, 0].any()) and not bool(first[:, :, 2].any()) and bool(first[:, :, 1].any())


def test_refusals_on_tensors():
    """A workspace one byte short and each unsupported channel combination are refused with a message, by the wrapper or by the
    entry point behind it."""
    from lidarnerf import unet_train as ut

    def t(*shape):
        return torch.zeros(shape, dtype=torch.float16, device="cuda")

    src0, dz, dw = t(1, 17, 31, 64), t(1, 17, 31, 64), torch.zeros(64, 64, 3, 3, device="cuda")
    need = ut.conv3x3_backward_weight_workspace_bytes(1, 17, 31, False, 64, 0, 64)
    with pytest.raises(RuntimeError, match="workspace"):
        ut.conv3x3_backward_weight(src0, dz, torch.zeros(need - 1, dtype=torch.uint8, device="cuda"), dw)
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    ut.conv3x3_backward_weight(src0, dz, ws[:need], dw)
    for C0, C1, Cout, cin in ((96, 0, 64, 96), (64, 32, 64, 96), (32, 32, 64, 64), (128, 64, 64, 192), (64, 0, 96, 64), (64, 0, 32, 64),
                              (64, 0, 64, 10), (32, 0, 64, 33)):
        src1 = t(1, 17, 31, C1) if C1 else None
        with pytest.raises(RuntimeError, match="C0|C1|Cout|Cin"):
            ut.conv3x3_backward_weight(t(1, 17, 31, C0), t(1, 17, 31, Cout), ws, torch.zeros(Cout, cin, 3, 3, device="cuda"), src1=src1)
    with pytest.raises(RuntimeError, match="dweight"):
        ut.conv3x3_backward_weight(src0, t(1, 17, 30, 64), ws, dw)
    with pytest.raises(RuntimeError, match="second source"):
        ut.conv3x3_backward_weight(src0, dz, ws, torch.zeros(64, 128, 3, 3, device="cuda"), src1=t(1, 15, 31, 64))
    torch.cuda.synchronize()


@pytest.mark.parametrize("k", (1, 6), ids=("b", "e10"))
def test_an_inf_in_dz_stays_in_its_output_channel(k):
    """One infinite dz element makes exactly the 9 Cin entries of its co non-finite (inf times a zero of the operand or of the padding is
    a NaN) and leaves every other bit alone; nothing faults, nothing is written outside."""
    c = WC.wgrad_case(k)
    cin = WC.WGRAD_CASES[k][0] + WC.WGRAD_CASES[k][1]
    src0, src1, dz = _operands(c)
    clean = _run(c, src0, src1, dz, cin)
    co = 37
    dz = dz.clone()
    dz[0, 5, 11, co] = float("inf")
    for variant in VARIANTS:
        got = _run(c, src0, src1, dz, cin, variant)
        keep = torch.ones(dz.shape[3], dtype=torch.bool, device="cuda")
        keep[co] = False
        assert torch.equal(G._bits(got[keep]), G._bits(clean[keep])), variant
        assert not bool(torch.isfinite(got[co]).any()) and got[co].numel() == 9 * cin, variant


# ------------------------------------------------------------------------------------------------------ the whole net
CONV_NAMES = [n for n, s in R.state_spec() if len(s) == 4 and s[2] == 3]


@functools.lru_cache(maxsize=None)
def _conv_deviation():
    """Relative L2 distance, per 3 x 3 weight, of the stock net's own fp16-autocast CPU gradients (static scale 1024) from the float64
    restatement — the computation of test_unet_train_conv_gpu._reference for the 18 tensors it leaves out.  At that scale the stock
    run overflows fp16 in some of these tensors (autocast forms the weight gradient of a convolution in fp16: anything above 65504 is
    inf), so its deviation there is infinite and bounds nothing; for those tensors alone the deviation is taken from the same run at
    a static scale of 32, where nothing overflows — a relative distance does not depend on the scale otherwise.  Returns
    ({name: deviation}, names that needed the smaller scale)."""
    ref = TC._reference()

    def run(scale):
        stock = R.stock_unet()
        stock.load_state_dict(ref["sd"])
        stock.train()
        with torch.autocast("cpu", dtype=torch.float16):
            out = stock(ref["x"])
        out.backward((ref["cot"] * scale).to(out.dtype))
        params = dict(stock.named_parameters())
        return {n: float((params[n].grad.double() / scale - ref["grads"][n]).norm() / ref["grads"][n].norm()) for n in CONV_NAMES}

    dev = run(1024)
    overflowed = [n for n in CONV_NAMES if not dev[n] < float("inf")]
    if overflowed:
        small = run(32)
        dev.update({n: small[n] for n in overflowed})
    assert all(0 < dev[n] < float("inf") for n in CONV_NAMES)
    return dev, overflowed


@functools.lru_cache(maxsize=None)
def _full_run():
    from lidarnerf import unet_train as ut
    ref = TC._reference()
    net = TC._net(ref["sd"])
    x, d = ref["x"].cuda(), (ref["cot"] * 1024).float().cuda()
    _, state = ut.train_forward(net, x)
    part = {k: v.clone() for k, v in ut.train_backward(net, state, d).items()}
    net.load_state_dict(ref["sd"])
    _, state = ut.train_forward(net, x)
    full = {k: v.clone() for k, v in ut.train_backward(net, state, d, conv_weights=True).items()}
    torch.cuda.synchronize()
    return net, part, full


def test_all_64_gradients_against_the_float64_reference():
    """2 x 23 x 37, the G18 hashed batch, cotangent x 1024 — the setting and the rule of
    test_whole_net_gradients_against_the_float64_reference.  All 64 names, f32, the parameter's shape; the 46 that existed have the
    bits of a run without the convolution weights; each of the 18 new ones is within 2 x the stock net's own fp16-autocast CPU
    deviation for that tensor, in relative L2 against unet_backward_from_state (_conv_deviation: where that deviation is infinite
    because the stock run overflows fp16, the same run at scale 32 gives it).  Measured on an MI355X: the largest ratio deviation /
    bound is 0.505 (down4's second convolution, 0.454 of 0.900), the smallest 0.462; inc.double_conv.0.weight 0.457 of 0.953,
    up4.conv.double_conv.3.weight 0.064 of 0.132."""
    ref, (dev, overflowed) = TC._reference(), _conv_deviation()
    print("the stock run at scale 1024 overflows fp16 in (bound from its run at scale 32):", overflowed)
    net, part, full = _full_run()
    spec = dict(R.state_spec())
    assert len(CONV_NAMES) == 18 and set(part) == set(K.GRAD_NAMES) and len(part) == 46
    assert set(full) == set(K.GRAD_NAMES) | set(CONV_NAMES) == {n for n, _ in net.named_parameters()} and len(full) == 64
    for name, g in full.items():
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(spec[name]), name
    for name in K.GRAD_NAMES:
        assert torch.equal(G._bits(full[name]), G._bits(part[name])), name
    ratios = {}
    for name in CONV_NAMES:
        want = ref["grads"][name]
        d = float((full[name].double().cpu() / 1024 - want).norm() / want.norm())
        ratios[name] = (d, 2 * dev[name])
        print(f"{name}: deviation {d:.4g}, bound {2 * dev[name]:.4g}, ratio {d / (2 * dev[name]):.3f}")
    print(f"largest ratio {max(d / b for d, b in ratios.values()):.3f}")
    for name, (d, bound) in ratios.items():
        assert d <= bound, (name, d, bound)


def test_full_backward_allocates_once_and_never_waits():
    """On the integer-valued net: the second forward + full backward allocates nothing and never synchronises, from a workspace filled
    with 0xff, and gives the first call's bits."""
    from lidarnerf import unet_train as ut
    x = R.integer_image(2900, (2, 10, 23, 37)).cuda()
    net = TC._net(R.integer_state_dict(), eps=0.0)
    d = T.g18_train_cotangent().float().cuda()
    _, state = ut.train_forward(net, x)
    first = {k: v.clone() for k, v in ut.train_backward(net, state, d, conv_weights=True).items()}
    assert len(first) == 64
    net.load_state_dict(R.integer_state_dict())
    state["raw"].fill_(255)
    torch.cuda.synchronize()
    net._packed = None
    before = torch.cuda.memory_stats()["allocation.all.allocated"], torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, state2 = ut.train_forward(net, x)
        grads = ut.train_backward(net, state2, d, conv_weights=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (torch.cuda.memory_stats()["allocation.all.allocated"], torch.cuda.memory_allocated()) == before and state2 is state
    for name in first:
        assert torch.equal(G._bits(first[name]), G._bits(grads[name])), name


def test_captured_replay_of_the_full_backward_equals_eager():
    from lidarnerf import unet_train as ut
    ref = TC._reference()
    _, _, eager = _full_run()
    x, d = ref["x"].cuda(), (ref["cot"] * 1024).float().cuda()
    net = TC._net(ref["sd"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        state = ut.train_forward(net, x)[1]
        ut.train_backward(net, state, d, conv_weights=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = ut.train_backward(net, ut.train_forward(net, x)[1], d, conv_weights=True)
    for _ in range(2):
        net.load_state_dict(ref["sd"])
        state["raw"].fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        assert len(grads) == 64
        for name, g in grads.items():
            assert torch.equal(G._bits(g), G._bits(eager[name])), name
