"""The training-mode convolution layer of the ray-drop U-Net on the device (csrc/unet_train_conv.hip, the RAW epilogue of csrc/unet.hip,
lidarnerf/unet_train.py: train_forward / train_backward) in the habits of tests/test_unet_gpu.py: every output NaN-filled before the
call and followed by guard words, every call made twice with equal bits, torch.equal wherever the problem has one answer
(tests/test_unet_train_conv_cpu.py asserts the conditions).  Where a bound is used it comes from the rounding model written down in
DESIGN §19 or from the stock net's own fp16-autocast run on the CPU, never from the device; every such test prints its figures before
it asserts."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_unet_gpu as G
import unet_ref as R
import unet_train_conv_cases as K
import unet_train_ref as T

pytestmark = pytest.mark.gpu


def _nhwc(x):
    """float64 NCHW on the host -> fp16 NHWC on the device, no channel padding."""
    return x.permute(0, 2, 3, 1).to(torch.float16).contiguous().cuda()


def _vec(x):
    return x.float().cuda()


# ------------------------------------------------------------------------------------------------------ the raw convolution
@pytest.mark.parametrize("index", range(len(R.CONV_CASES)))
def test_conv3x3_raw_exact(index):
    """The 18 operands of unet_ref.CONV_CASES with every tile against the integer-exact sums themselves: pool on read, the second
    source with its padding, N = 2 — and negative sums, which the ReLU epilogue never shows."""
    from lidarnerf import unet_train as ut
    C0, C1, Cout, H, W, pool, off, N = R.CONV_CASES[index]
    c = R.conv_case(index)
    src0 = G.nhwc16(c["src0"])
    src1 = G.nhwc16(c["src1"]) if C1 else None
    wimg = G.conv_weight_image(c["weight"], C0)
    want = F.conv2d(c["x"], c["weight"].double(), padding=1).permute(0, 2, 3, 1).contiguous().cuda()
    assert bool((want < 0).any())
    first = None
    for tile in G.TILES:
        outs = []
        for _ in range(2):
            out, guard = G.guarded((N, H, W, Cout), torch.float16)
            ut.conv3x3_raw(src0, wimg, out, src1=src1, pool=bool(pool), tile=tile)
            assert torch.equal(out.double(), want), (tile, int((out.double() != want).sum()))
            assert G.guard_ok(guard), tile
            outs.append(out)
        first = outs[0] if first is None else first
        assert torch.equal(G._bits(outs[0]), G._bits(outs[1])) and torch.equal(G._bits(outs[0]), G._bits(first))


@pytest.mark.parametrize("k", range(len(K.DGRAD_CASES)))
def test_data_gradient_exact(k):
    """dx = conv3x3_raw(dz, bwd) with the image packed on the device, against conv_transpose2d on sparse integer weights: 64 -> 64 at
    15 x 17 and 1 x 257, 128 -> 64 + 64 at 16 x 16 and 17 x 17, 1024 -> 512 at 2 x 3, N = 2; every tile."""
    from lidarnerf import unet_train as ut
    Cout, C0, C1, H, W, N = K.DGRAD_CASES[k]
    c = K.dgrad_case(k)
    fwd = torch.empty(Cout, 9, C0 + C1, dtype=torch.float16, device="cuda")
    bwd, g0 = G.guarded((C0 + C1, 9, Cout), torch.float16)
    ut.pack_conv3x3(c["weight"].float().cuda(), fwd, bwd)
    dz = _nhwc(c["dz"])
    want = c["want"].permute(0, 2, 3, 1).contiguous().cuda()
    first = None
    for tile in G.TILES:
        outs = []
        for _ in range(2):
            dx, guard = G.guarded((N, H, W, C0 + C1), torch.float16)
            ut.conv3x3_raw(dz, bwd, dx, tile=tile)
            assert torch.equal(dx.double(), want), (tile, int((dx.double() != want).sum()))
            assert G.guard_ok(guard) and G.guard_ok(g0)
            outs.append(dx)
        first = outs[0] if first is None else first
        assert torch.equal(G._bits(outs[0]), G._bits(outs[1])) and torch.equal(G._bits(outs[0]), G._bits(first))


def test_data_gradient_feeds_pool_backward_and_upconv_backward_in_place():
    """The concatenating layer's dx [1, 17, 17, 64 + 64] is read in place by the existing kernels: pool_backward takes channels [0, 64)
    as the skip gradient (pixel stride 128), upconv2x2_backward_data channels [64, 128) of the 16 x 16 corner (a padded row and column
    dropped)."""
    from lidarnerf import unet_train as ut
    k = len(K.DGRAD_CASES) - 1
    Cout, C0, C1, H, W, N = K.DGRAD_CASES[k]
    assert (H, W, C0, C1) == (17, 17, 64, 64)
    c = K.dgrad_case(k)
    fwd = torch.empty(Cout, 9, C0 + C1, dtype=torch.float16, device="cuda")
    bwd = torch.empty(C0 + C1, 9, Cout, dtype=torch.float16, device="cuda")
    ut.pack_conv3x3(c["weight"].float().cuda(), fwd, bwd)
    dcat = torch.empty(N, H, W, C0 + C1, dtype=torch.float16, device="cuda")
    ut.conv3x3_raw(_nhwc(c["dz"]), bwd, dcat)
    x = R.integer_image(7190, (N, C0, H, W)).double()
    dpool = R.integer_image(7191, (N, C0, H // 2, W // 2), top=4).double() - 2
    want = T.pool_backward(x, dpool, c["want"][:, :C0])
    assert torch.equal(want, R.q16(want))
    dx, guard = G.guarded((N, H, W, C0), torch.float16)
    ut.pool_backward(_nhwc(x), _nhwc(dpool), dx, dskip=dcat)
    assert torch.equal(dx.double(), want.permute(0, 2, 3, 1).contiguous().cuda()) and G.guard_ok(guard)
    w = R.sparse_weight(7192, (128, C1, 2, 2), 16, 128).double()
    want = T.upconv_backward(torch.zeros(N, 128, H // 2, W // 2, dtype=torch.float64), w, c["want"][:, C0:, :16, :16])[0]
    bound = float(T.upconv_backward(torch.zeros(N, 128, 8, 8, dtype=torch.float64), w.abs(), c["want"][:, C0:, :16, :16].abs())[0].max())
    assert bound < 2 ** 24 and want.unique().numel() > 20
    ufwd = torch.empty(4, C1, 128, dtype=torch.float16, device="cuda")
    ubwd = torch.empty(128, 4, C1, dtype=torch.float16, device="cuda")
    ut.pack_upconv(w.float().cuda(), ufwd, ubwd)
    dup, guard = G.guarded((N, H // 2, W // 2, 128), torch.float16)
    ut.upconv2x2_backward_data(dcat, ubwd, dup, offset=C0)
    assert torch.equal(dup.double(), R.q16(want).permute(0, 2, 3, 1).contiguous().cuda()) and G.guard_ok(guard)


@pytest.mark.parametrize("k", range(len(K.PACK_CASES)))
def test_pack_exact(k):
    """Both images for Cin = 10 -> 32 (forward only: the first layer needs no data gradient), 64, 128 and 1024."""
    from lidarnerf import unet_train as ut
    Cout, Cin = K.PACK_CASES[k]
    w = K.pack_weight(k)
    want_fwd, want_bwd = K.pack_images(w)
    for _ in range(2):
        fwd, g0 = G.guarded(tuple(want_fwd.shape), torch.float16)
        if Cin % 64:
            ut.pack_conv3x3(w.cuda(), fwd)
            assert torch.equal(fwd.cpu(), want_fwd) and G.guard_ok(g0)
            with pytest.raises(RuntimeError, match="bwd"):
                ut.pack_conv3x3(w.cuda(), fwd, torch.empty(Cin, 9, Cout, dtype=torch.float16, device="cuda"))
        else:
            bwd, g1 = G.guarded(tuple(want_bwd.shape), torch.float16)
            ut.pack_conv3x3(w.cuda(), fwd, bwd)
            assert torch.equal(fwd.cpu(), want_fwd) and torch.equal(bwd.cpu(), want_bwd) and G.guard_ok(g0) and G.guard_ok(g1)


# ------------------------------------------------------------------------------------------------------ BatchNorm, exact
def _run_bn(c, z=None, in_place=False):
    """bn_stats -> bn_relu -> bn_relu_backward on the [M, C] problem `c` with guarded, NaN-filled outputs and workspaces; eps = 0,
    momentum = 0.5."""
    from lidarnerf import unet_train as ut
    M, Cc = c["M"], c["C"]
    shape = (1, 1, M, Cc)
    z = (c["z"] if z is None else z).to(torch.float16).cuda().reshape(shape)
    out, guards = {}, []
    for name in ("mean", "invstd", "scale", "shift", "dgamma", "dbeta"):
        out[name], g = G.guarded((Cc,), torch.float32)
        guards.append(g)
    for name in ("a", "dz"):
        out[name], g = G.guarded(shape, torch.float16)
        guards.append(g)
    ws, g = G.guarded((ut.bn_stats_workspace_bytes(M, Cc) // 4,), torch.float32)
    guards.append(g)
    out["running_mean"], out["running_var"] = _vec(c["running_mean"]), _vec(c["running_var"])
    ut.bn_stats(z, _vec(c["gamma"]), _vec(c["beta"]), 0.0, K.BN_MOMENTUM, ws, out["mean"], out["invstd"], out["scale"], out["shift"],
                out["running_mean"], out["running_var"])
    ut.bn_relu(z, out["scale"], out["shift"], out["a"])
    ws.fill_(float("nan"))
    da = c["da"].to(torch.float16).cuda().reshape(shape)
    if in_place:
        out["dz"].copy_(da)
        da = out["dz"]
    ut.bn_relu_backward(z, out["a"], da, out["mean"], out["invstd"], out["scale"], ws, out["dz"], out["dgamma"], out["dbeta"])
    torch.cuda.synchronize()
    assert all(G.guard_ok(g) for g in guards)
    return out


@pytest.mark.parametrize("k", range(len(K.BN_CASES)))
def test_bn_exact(k):
    """z = m + sigma e with half of every channel at each sign: mean, invstd, scale, shift, a, dbeta, dgamma and dz have one value each
    and the device gives it, for M = 2, 64, 66, 1020 and 2^14 + 2 (one partial, several, a ragged last one, the doubled partial) and
    C = 32, 64, 96, 1024; running_mean exactly, running_var within one f32 ulp of the float64 value of 0.5 rv + 0.5 var M / (M - 1)
    (exactly where M - 1 is a power of two); dz written over da gives the same bits."""
    c = K.bn_case(k)
    M, Cc = c["M"], c["C"]
    runs = [_run_bn(c), _run_bn(c), _run_bn(c, in_place=True)]
    got = runs[0]
    for name in ("mean", "invstd", "scale", "shift", "dgamma", "dbeta"):
        assert torch.equal(got[name].double().cpu(), c[name]), (name, int((got[name].double().cpu() != c[name]).sum()))
    for name in ("a", "dz"):
        assert torch.equal(got[name].double().cpu().reshape(M, Cc), c[name]), (name, int((got[name].double().cpu().reshape(M, Cc) != c[name]).sum()))
    assert torch.equal(got["running_mean"].double().cpu(), c["want_running_mean"])
    rv, want = got["running_var"].double().cpu(), c["want_running_var"]
    ulp = torch.from_numpy(np.spacing(want.float().numpy()).astype(np.float64))
    print(f"running_var: largest distance {float(((rv - want).abs() / ulp).max()):.3f} f32 ulp of the float64 value (M = {M})")
    if ((M - 1) & (M - 2)) == 0:
        assert torch.equal(rv, want)
    assert bool(((rv - want).abs() <= ulp).all())
    for other in runs[1:]:
        for name in got:
            assert torch.equal(G._bits(got[name]), G._bits(other[name])), name


def test_bn_non_finite_values_stay_in_their_channel():
    """A NaN in one channel's z makes that channel's statistics NaN and leaves every other channel's bits alone; a constant channel with
    eps = 0 has variance 0 and a non-finite invstd; nothing faults, nothing is written outside the outputs."""
    c = K.bn_case(3)
    z = c["z"].clone()
    z[5, 7] = float("nan")
    z[:, 9] = 2.0
    clean, got = _run_bn(c), _run_bn(c, z=z)
    keep = torch.ones(c["C"], dtype=torch.bool, device="cuda")
    keep[7] = keep[9] = False
    for name in ("mean", "invstd", "scale", "shift", "dgamma", "dbeta", "running_mean", "running_var"):
        assert torch.equal(G._bits(got[name][keep]), G._bits(clean[name][keep])), name
    for name in ("a", "dz"):
        assert torch.equal(G._bits(got[name][..., keep]), G._bits(clean[name][..., keep])), name
    assert bool(torch.isnan(got["mean"][7])) and bool(torch.isnan(got["invstd"][7])) and bool(torch.isnan(got["running_var"][7]))
    assert float(got["mean"][9]) == 2.0 and not bool(torch.isfinite(got["invstd"][9]))


# ------------------------------------------------------------------------------------------------------ BatchNorm, general data
def test_bn_general_data_within_the_rounding_model():
    """Hashed z at 2 x 23 x 37 x 64 with one channel at |mean| = 100 sigma, against float64 of the same fp16 z; bounds: the rounding model
    of DESIGN §19 (tests/unet_train_conv_cases.py: bn_general_reference).  Measured on an MI355X, as the largest fraction of the bound
    any element uses: mean 0.92, invstd 0.90, scale 0.94, shift 0.88, a 0.99, dbeta 0.88, dgamma 0.03, dz 1.00 (0.997) — the bounds are
    one rounding of the stored format (half an ulp of fp16 for a and dz, of f32 for the vectors) plus summation terms that are far
    smaller, and among thousands of elements one comes close to half an ulp; dgamma's bound is dominated by its allowance for xhat."""
    from lidarnerf import unet_train as ut
    c = K.bn_general_case()
    ref = K.bn_general_reference(c)
    M, Cc = K.GENERAL_BN
    shape = (1, 1, M, Cc)
    z, da = c["z"].to(torch.float16).cuda().reshape(shape), c["da"].to(torch.float16).cuda().reshape(shape)
    out = {name: G.guarded((Cc,), torch.float32) for name in ("mean", "invstd", "scale", "shift", "dgamma", "dbeta")}
    a, ga = G.guarded(shape, torch.float16)
    dz, gz = G.guarded(shape, torch.float16)
    ws, gw = G.guarded((ut.bn_stats_workspace_bytes(M, Cc) // 4,), torch.float32)
    ut.bn_stats(z, _vec(c["gamma"]), _vec(c["beta"]), c["eps"], 0.1, ws, *[out[n][0] for n in ("mean", "invstd", "scale", "shift")])
    ut.bn_relu(z, out["scale"][0], out["shift"][0], a)
    ut.bn_relu_backward(z, a, da, out["mean"][0], out["invstd"][0], out["scale"][0], ws, dz, out["dgamma"][0], out["dbeta"][0])
    torch.cuda.synchronize()
    assert all(G.guard_ok(g) for g in [ga, gz, gw] + [v[1] for v in out.values()])
    frac = {}
    for name in ("mean", "invstd", "scale", "shift", "dbeta", "dgamma"):
        frac[name] = float(((out[name][0].double().cpu() - ref[name]).abs() / ref["bound"][name]).max())
    # a from the device's own f32 scale / shift: one fmaf rounding and one fp16 rounding away from the float64 value
    v = c["z"] * out["scale"][0].double().cpu() + out["shift"][0].double().cpu()
    frac["a"] = float(((a.double().cpu().reshape(M, Cc) - torch.relu(v)).abs() / (2.0 ** -11 * v.abs() * (1 + 2.0 ** -12) + 2.0 ** -25)).max())
    # dz where the device's ReLU mask is the reference's (an a that rounds to 0 on one side only is a different, equally valid g)
    same = (a.double().cpu().reshape(M, Cc) > 0) == (ref["a"] > 0)
    assert float(same.double().mean()) > 0.999
    frac["dz"] = float((((dz.double().cpu().reshape(M, Cc) - ref["dz"]).abs() / ref["bound"]["dz"])[same]).max())
    print("fraction of the bound used:", {k: round(v, 4) for k, v in frac.items()})
    for name, f in frac.items():
        assert f <= 1.0, (name, f)


# ------------------------------------------------------------------------------------------------------ the whole net
def _net(sd, eps=None):
    from lidarnerf.unet import RayDropUNet
    net = RayDropUNet()
    if eps is not None:
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eps = eps
    net.load_state_dict(sd)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _reference():
    """Float64 logits, running statistics and gradients of the G18 batch, and the deviation from them of the stock net's own CPU run
    under fp16 autocast with a static loss scale of 1024 — per tensor: max-norm for logits and running statistics, relative L2 for
    gradients."""
    sd, x, cot = R.hash_state_dict(), T.g18_train_batch(), T.g18_train_cotangent()
    logits, state = T.unet_train_forward(sd, x)
    grads = T.unet_backward_from_state(sd, state, cot)
    stock = R.stock_unet()
    stock.load_state_dict(sd)
    stock.train()
    with torch.autocast("cpu", dtype=torch.float16):
        out = stock(x)
    out.backward((cot * 1024).to(out.dtype))
    dev = {"logits": float((out.detach().double() - logits).abs().max())}
    for name, p in stock.named_parameters():
        if name in K.GRAD_NAMES:
            dev[name] = float((p.grad.double() / 1024 - grads[name]).norm() / grads[name].norm())
    buffers = dict(stock.named_buffers())
    for name, want in state["running"].items():
        dev[name] = float((buffers[name].double() - want).abs().max())
    return {"sd": sd, "x": x, "cot": cot, "logits": logits, "running": state["running"], "grads": grads, "dev": dev}


@functools.lru_cache(maxsize=None)
def _device_run():
    from lidarnerf import unet_train as ut
    ref = _reference()
    net = _net(ref["sd"])
    logits, state = ut.train_forward(net, ref["x"].cuda())
    grads = ut.train_backward(net, state, (ref["cot"] * 1024).float().cuda())
    torch.cuda.synchronize()
    return net, logits.clone(), state, {k: v.clone() for k, v in grads.items()}


def test_whole_net_forward_against_the_float64_reference():
    """2 x 23 x 37, the G18 hashed batch.  Logits within 2 x the reference's recorded autocast deviation (G18: 0.029), every running
    statistic within 2 x the stock net's autocast deviation for that tensor; num_batches_tracked counts.  Measured on an MI355X:
    logits 0.0291 of a bound of 0.0588; running statistics at most 0.62 of their bounds."""
    ref = _reference()
    net, logits, state, _ = _device_run()
    g18 = np.load(os.path.join(G.GOLDEN, "g18_unet_train.npz"))
    dev = float((logits.double().cpu() - ref["logits"]).abs().max())
    print(f"train-mode logits: deviation {dev:.4g}, bound {2 * float(g18['dev_amp16']):.4g}")
    assert dev <= 2 * float(g18["dev_amp16"])
    sd = net.state_dict()
    worst = 0.0
    for name, want in ref["running"].items():
        d = float((sd[name].double().cpu() - want).abs().max())
        worst = max(worst, d / (2 * ref["dev"][name]))
        assert d <= 2 * ref["dev"][name], (name, d, ref["dev"][name])
    print(f"running statistics: largest fraction of 2 x the autocast deviation {worst:.3f}")
    assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked")) and not net.training
    assert len(state["layers"]) == 18 and all(l["dz"].shape == l["z"].shape and l["operand"][0] is not None for l in state["layers"])


def test_whole_net_gradients_against_the_float64_reference():
    """The 46 gradients for the G18 cotangent scaled by 1024, divided by it again, in relative L2 against unet_backward_from_state; bound
    per tensor: 2 x the deviation of the stock net's own fp16-autocast CPU run (static scale 1024).  The 18 convolution weights are
    absent.  Measured on an MI355X: the largest ratio deviation / bound is 0.60 (outc.conv.weight, 0.0107 of 0.0180), the smallest non-trivial one 0.44;
    inc.double_conv.1.weight 0.381 of 0.749, down4's last BatchNorm weight 0.226 of 0.460, up1.up.weight 0.228 of 0.454."""
    ref = _reference()
    _, _, _, grads = _device_run()
    assert set(grads) == set(K.GRAD_NAMES) and len(grads) == 46 and not any(n.endswith((".0.weight", ".3.weight")) for n in grads)
    ratios = {}
    for name in K.GRAD_NAMES:
        want = ref["grads"][name]
        got = grads[name].double().cpu() / 1024
        assert got.shape == want.shape and grads[name].dtype == torch.float32, name
        d = float((got - want).norm() / want.norm())
        ratios[name] = (d, 2 * ref["dev"][name])
        print(f"{name}: deviation {d:.4g}, bound {2 * ref['dev'][name]:.4g}")
    for name, (d, bound) in ratios.items():
        assert d <= bound, (name, d, bound)


def _hand_chained(net, x):
    """train_forward through the entry points on separate tensors: (logits, running statistics after the call)."""
    from lidarnerf import unet, unet_train as ut
    N, _, H, W = x.shape
    sizes = unet.level_sizes(H, W)
    bufs = {"input": unet.unet_input(x, torch.empty(N, H, W, 32, dtype=torch.float16, device="cuda"))}

    def vec(Cc):
        return torch.empty(Cc, device="cuda")

    cur = None
    for k, lay in enumerate(ut.train_layers()):
        h, w = sizes[lay["level"]]
        if lay["src1"] is not None:
            up = net.get_submodule(f"up{(k - 10) // 2 + 1}.up")
            cin = up.weight.shape[0]
            ufwd = torch.empty(4, cin // 2, cin, dtype=torch.float16, device="cuda")
            ut.pack_upconv(up.weight.detach(), ufwd)
            bufs[lay["src1"]] = unet.upconv2x2(cur, ufwd, up.bias.detach(),
                                               torch.empty(N, 2 * (h // 2), 2 * (w // 2), cin // 2, dtype=torch.float16, device="cuda"))
        conv, bn = net.get_submodule(lay["conv"]), net.get_submodule(lay["bn"])
        cout, cin = conv.weight.shape[:2]
        fwd = torch.empty(cout, 9, max(32, cin), dtype=torch.float16, device="cuda")
        ut.pack_conv3x3(conv.weight.detach(), fwd)
        z = torch.empty(N, h, w, cout, dtype=torch.float16, device="cuda")
        ut.conv3x3_raw(bufs[lay["src0"]], fwd, z, src1=None if lay["src1"] is None else bufs[lay["src1"]], pool=lay["pool"])
        mean, invstd, scale, shift = vec(cout), vec(cout), vec(cout), vec(cout)
        ws = torch.empty(ut.bn_stats_workspace_bytes(N * h * w, cout), dtype=torch.uint8, device="cuda")
        ut.bn_stats(z, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, ws, mean, invstd, scale, shift, bn.running_mean,
                    bn.running_var)
        cur = bufs[lay["out"]] = ut.bn_relu(z, scale, shift, torch.empty_like(z))
        bn.num_batches_tracked.add_(1)
    logits = torch.empty(N, 1, H, W, device="cuda")
    unet.head(cur, net.outc.conv.weight.detach().reshape(64).half(), net.outc.conv.bias.detach(), logits)
    return logits


def test_train_forward_is_the_chain_of_entry_points_and_allocates_once():
    """On the integer-valued net (batch statistics are no integers there, so only this is checked): train_forward equals the
    hand-chained entry points bit for bit, logits and running statistics.  The second call allocates nothing and never waits for the
    device, train_backward likewise; a NaN-filled workspace changes nothing."""
    from lidarnerf import unet_train as ut
    x = R.integer_image(2900, (2, 10, 23, 37)).cuda()
    a, b = _net(R.integer_state_dict(), eps=0.0), _net(R.integer_state_dict(), eps=0.0)
    want = _hand_chained(a, x)
    got, state = ut.train_forward(b, x)
    assert torch.equal(G._bits(got), G._bits(want))
    sa, sb = a.state_dict(), b.state_dict()
    for name in sa:
        assert torch.equal(G._bits(sa[name].reshape(-1)), G._bits(sb[name].reshape(-1))), name
    d = T.g18_train_cotangent().float().cuda()
    first = {k: v.clone() for k, v in ut.train_backward(b, state, d).items()}
    b.load_state_dict(R.integer_state_dict())  # the same statistics going in
    state["raw"].fill_(255)
    torch.cuda.synchronize()
    b._packed = None  # (what load_state_dict packed for inference: train_forward drops it, which would show as freed memory)
    before = torch.cuda.memory_stats()["allocation.all.allocated"], torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again, state2 = ut.train_forward(b, x)
        grads = ut.train_backward(b, state2, d)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (torch.cuda.memory_stats()["allocation.all.allocated"], torch.cuda.memory_allocated()) == before
    assert state2 is state and again.data_ptr() == got.data_ptr() and torch.equal(G._bits(again), G._bits(want))
    for name in first:
        assert torch.equal(G._bits(first[name]), G._bits(grads[name])), name


def test_captured_replay_equals_eager():
    from lidarnerf import unet_train as ut
    ref = _reference()
    x, d = ref["x"].cuda(), (ref["cot"] * 1024).float().cuda()
    net = _net(ref["sd"])
    logits, state = ut.train_forward(net, x)
    eager = [logits.clone()] + [v.clone() for v in ut.train_backward(net, state, d).values()]
    eager_running = {k: v.clone() for k, v in net.state_dict().items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ut.train_backward(net, ut.train_forward(net, x)[1], d)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = ut.train_backward(net, ut.train_forward(net, x)[1], d)
    for _ in range(2):
        net.load_state_dict(ref["sd"])
        state["raw"].fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        for p, q in zip(eager, [state["logits"]] + list(grads.values())):
            assert torch.equal(G._bits(p), G._bits(q))
        for k, v in net.state_dict().items():
            assert torch.equal(G._bits(v.reshape(-1)), G._bits(eager_running[k].reshape(-1))), k


def test_inference_after_train_forward_uses_the_updated_statistics():
    from lidarnerf import unet_train as ut
    ref = _reference()
    x = ref["x"].cuda()
    net = _net(ref["sd"])
    before = net(x).clone()
    ut.train_forward(net, x)
    after = net(x).clone()
    fresh = _net({k: v.cpu() for k, v in net.state_dict().items()})
    assert torch.equal(G._bits(after), G._bits(fresh(x))) and not torch.equal(before, after)
    with pytest.raises(RuntimeError, match="training mode"):
        net.train()(x)
