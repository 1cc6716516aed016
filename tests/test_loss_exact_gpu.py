"""Known-answer tests of the three loss kernels every training step ends in — lnh_lidar_loss, lnh_lidar_loss_patch and
lnh_lidar_loss_ex (csrc/lidar_glue.hip) — through the C ABI: the loss and the two cotangents d loss / d depth, d loss / d image
that the whole backward pass starts from.

Problems, float64 reference and bounds: tests/loss_exact_cases.py (conditions asserted on the CPU by
tests/test_loss_exact_cpu.py; DESIGN.md section 8, "Exact tests of the loss kernels").  Inputs are dyadic, so no mask can flip
between kernel and reference.  TIER A (every mean over a power of two of elements, L1 / MSE / HUBER, SPATIAL, TV): one right
float32 value in any summation order, torch.equal on the loss and both gradients, and the same bits from every entry point
that states the same loss.  TIER B (other counts, BCE, GRAD_NORM_SMOOTH, COS): every element within K * 2^-24 * A of float64, A
the sum of |addends| of that element, K counted on the kernel text; ties and degenerate patches carry closed forms that are
compared exactly.  Each bounded test prints the largest error / (2^-24 A) it sees beside K.
Discipline of tests/exact_util.py: NaN-filled outputs with guard words, a NaN-filled guarded workspace of exactly
lnh_lidar_loss_ex_workspace_bytes(N), NaN rows behind depth, image and gt, every call twice with identical bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_exact_cases as lc
from exact_util import SENT, Out, _poisoned, _twice

pytestmark = pytest.mark.gpu
NAN = float("nan")
NAMES = lc.all_names()
TIER_A = [n for n in NAMES if lc.get_case(n).tier == "A"]
TIER_B = [n for n in NAMES if lc.get_case(n).tier == "B"]


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


class Problem:
    """The device side of a case: inputs with NaN rows behind them, the C struct of its options."""

    def __init__(self, c):
        from lidarnerf import _hip
        self.c = c
        self.depth, self.image, self.gt = _poisoned(_f32(c.depth), 1), _poisoned(_f32(c.image), 2), _poisoned(_f32(c.gt), 3)
        a = c.alphas
        self.opts = _hip.LidarLossOptionsC(*c.crit, c.flags, c.px, c.py, c.scale, c.delta, a["a_d"], a["a_r"], a["a_i"], a["a_g"],
                                           a["a_gn"], a["a_sp"], a["a_tv"])
        self.ws_bytes = int(_hip.lib().lnh_lidar_loss_ex_workspace_bytes(c.N))
        assert self.ws_bytes == lc.workspace_bytes(c.N)

    def run(self, entry, grad_scale=None, n=None):
        """One call on fresh NaN-filled buffers: (loss, g_depth, g_image, workspace)."""
        from gpu_util import call
        c, N = self.c, self.c.N if n is None else n
        rows = max(c.N, 8) if n is not None else c.N
        loss, gd, gi = Out((1,), torch.float32, fill=NAN), Out((rows,), torch.float32, fill=NAN), Out((rows, 2), torch.float32, fill=NAN)
        a, ws = c.alphas, None
        if entry == "ray":
            call("lnh_lidar_loss", self.depth, self.image, self.gt, N, a["a_d"], a["a_r"], a["a_i"], grad_scale, loss.buf,
                 gd.buf, gi.buf)
        elif entry == "patch":
            call("lnh_lidar_loss_patch", self.depth, self.image, self.gt, N, c.px, c.py, c.scale, a["a_d"], a["a_r"], a["a_i"],
                 a["a_g"], grad_scale, loss.buf, gd.buf, gi.buf)
        else:
            nbytes = self.ws_bytes if n is None else lc.workspace_bytes(n)
            ws = Out((nbytes // 4,), torch.float32, fill=NAN)
            call("lnh_lidar_loss_ex", self.depth, self.image, self.gt, N, C.byref(self.opts), grad_scale, ws.buf, nbytes,
                 loss.buf, gd.buf, gi.buf)
        torch.cuda.synchronize()
        for o, what in ((loss, "loss"), (gd, "g_depth"), (gi, "g_image"), (ws, "workspace")):
            if o is not None:
                assert bool((o.buf[o.n:] == SENT).all()), f"{c.name} {entry}: guard words behind {what} were overwritten"
        return loss, gd, gi, ws


def _host(o):
    return o.data().double().cpu().numpy()


def _closed(c, gd, gi, what):
    for name, out in (("g_depth", gd), ("g_image", gi)):
        if name in c.closed:
            idx, val = c.closed[name]
            got = _host(out)[idx]
            assert np.array_equal(got, val), f"{what}: {name} differs from its closed form at {np.argwhere(got != val)[:4].tolist()}"


# ================================================================================================ tier A: exact bits
@pytest.mark.parametrize("name", TIER_A)
def test_tier_a_exact_bits(name):
    c, r = lc.get_case(name), lc.ref_of(name)
    p = Problem(c)
    first = None
    for entry in c.entries():
        loss, gd, gi, _ = _twice(lambda: p.run(entry))
        what = f"{name} [{entry}]"
        loss.check(_f32([r.loss]), what + " loss")
        gd.check(_f32(r.g_depth), what + " g_depth")
        gi.check(_f32(r.g_image), what + " g_image")
        if first is None:
            first = (loss, gd, gi)
        else:   # every entry point that states this loss returns the same bits
            for u, v in zip(first, (loss, gd, gi)):
                assert torch.equal(_bits(u.buf), _bits(v.buf)), what + ": differs from lnh_lidar_loss_ex"
    assert len(c.entries()) == 2 or not c.is_default


def test_ray_and_ex_gradients_agree_bit_for_bit_on_a_random_batch():
    """Not dyadic: g_image and (px = 1: all of) g_depth of lnh_lidar_loss and lnh_lidar_loss_ex are the same bits on any problem —
    (2 a) d and a (2 d) round alike and both form 1.0f / (float)N the same way.  The two losses agree within their bounds."""
    g = torch.Generator().manual_seed(5)
    N = 4099
    gr = (torch.rand(N, generator=g) < 0.8).double()
    gt = torch.stack([gr, torch.rand(N, generator=g).double(), 0.5 + 70 * torch.rand(N, generator=g).double()], -1).float()
    depth = gt[:, 2] * (1 + 0.03 * torch.randn(N, generator=g))
    image = torch.rand(N, 2, generator=g)
    al = dict(lc.FIXED_ALPHAS, a_d=1000.0, a_r=1.0, a_i=10.0)
    c = lc.Case("random", 1, 1, lc.DEFAULT_CRIT, 0, 1.0, 0.25, al, depth.numpy(), image.numpy(), gt.numpy(), None)
    p = Problem(c)
    a = _twice(lambda: p.run("ray"))
    b = _twice(lambda: p.run("ex"))
    assert torch.equal(_bits(a[1].buf), _bits(b[1].buf)) and torch.equal(_bits(a[2].buf), _bits(b[2].buf))
    r = lc.reference(c)
    for entry, out in (("ray", a), ("ex", b)):
        ql, qd, qi = lc.ratios(_host(out[0])[0], _host(out[1]), _host(out[2]), r)
        print(f"random [{entry}]: loss {ql:.2f} (K {lc.k_loss(c, entry)}), g_depth {qd:.2f}, g_image {qi:.2f}")
        assert ql <= lc.k_loss(c, entry) and qd <= lc.k_gdepth(c, entry) and qi <= lc.k_gimage(c, entry)


# ================================================================================================ tier B: bounded
@pytest.mark.parametrize("name", TIER_B)
def test_tier_b_within_the_derived_bound(name):
    c, r = lc.get_case(name), lc.ref_of(name)
    p = Problem(c)
    for entry in c.entries():
        loss, gd, gi, _ = _twice(lambda: p.run(entry))
        what = f"{name} [{entry}]"
        got = _host(loss)[0], _host(gd), _host(gi)
        assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all(), what + ": not finite"
        ql, qd, qi = lc.ratios(*got, r)
        kl, kd, ki = lc.k_loss(c, entry), lc.k_gdepth(c, entry), lc.k_gimage(c, entry)
        print(f"{what}: error / (2^-24 A): loss {ql:.2f} (K {kl}), g_depth {qd:.2f} (K {kd}), g_image {qi:.2f} (K {ki})")
        assert ql <= kl, f"{what}: loss {got[0]!r} against {r.loss!r}: {ql:.1f} > K = {kl}"
        assert qd <= kd, f"{what}: g_depth off by {qd:.1f} * 2^-24 A > K = {kd}"
        assert qi <= ki, f"{what}: g_image off by {qi:.1f} * 2^-24 A > K = {ki}"
        _closed(c, gd, gi, what)


# ================================================================================================ N = 0
@pytest.mark.parametrize("entry", ["ray", "patch", "ex"])
def test_no_rays_writes_a_zero_loss_and_nothing_else(entry):
    c = lc.get_case("2x2x5_default")
    loss, gd, gi, ws = _twice(lambda: Problem(c).run(entry, n=0))
    assert float(loss.data()[0]) == 0.0
    assert bool(torch.isnan(gd.data()).all()) and bool(torch.isnan(gi.data()).all()), "a gradient buffer was touched at N = 0"
    assert ws is None or ws.n == 0


# ================================================================================================ locality
STRADDLING = (255, 270)   # rays of patch 17 of the 3 x 5 cases: it lies across the first two workgroups


@pytest.mark.parametrize("config", ["cos_all", "l1_sobel_all", "cos_sobel", "default"])
def test_a_changed_depth_stays_inside_its_patch(config):
    """Two runs whose bits are compared: one ray of the straddling patch gets another depth, then NaN.  The gradient of every
    other patch — its two neighbours included — and all of g_image keep their bits; with NaN the loss is NaN and the patch's own
    g_depth is not finite (but for the default loss: every derivative of its L1 terms is a sign, and sign(NaN) = 0)."""
    c = lc.get_case(lc.STRADDLE + config)
    lo, hi = STRADDLING
    ray = next(n for n in range(lo + 6, hi) if c.gt[n, 0] == 1.0)   # a returned ray of the patch's middle row
    assert c.S == 15 and lo == 17 * c.S and lo < lc.WG < hi
    outside = torch.ones(c.N, dtype=torch.bool, device="cuda")
    outside[lo:hi] = False
    for entry in c.entries():
        base = _twice(lambda: Problem(c).run(entry))
        moved = _twice(lambda: Problem(c.replace_depth(ray, c.depth[ray] + 3 * c.scale * 2.0 ** -12)).run(entry))
        nan = _twice(lambda: Problem(c.replace_depth(ray, NAN)).run(entry))
        what = f"{c.name} [{entry}]"
        for other, label in ((moved, "a changed depth"), (nan, "a NaN depth")):
            assert torch.equal(_bits(base[1].data())[outside], _bits(other[1].data())[outside]), f"{what}: {label} reached another patch"
            assert torch.equal(_bits(base[2].buf), _bits(other[2].buf)), f"{what}: {label} reached g_image"
        assert not torch.equal(_bits(base[1].data())[lo:hi], _bits(moved[1].data())[lo:hi]), what + ": the change had no effect at all"
        assert bool(torch.isnan(nan[0].data()).all()), what + ": loss of a NaN depth"
        assert config == "default" or not bool(torch.isfinite(nan[1].data()[lo:hi]).all()), what + ": g_depth of the patch with the NaN is finite"


# ================================================================================================ grad_scale
@pytest.mark.parametrize("name", ["A_ray1024_0", "A_2x2x256_default", "A_4x4x32_mse", "3x5x35_cos_sobel", "2x8x65_default",
                                  "17x16x2_bce_sobel_gn"])
def test_grad_scale(name):
    """A null pointer and a device 1.0 give the same bits; 2^16 multiplies every gradient element by exactly 2^16 (the elements
    stay normal numbers) and leaves the loss alone."""
    c = lc.get_case(name)
    p = Problem(c)
    one, big = torch.ones((), device="cuda"), torch.full((), 65536.0, device="cuda")
    for entry in c.entries():
        a = _twice(lambda: p.run(entry))
        b = _twice(lambda: p.run(entry, grad_scale=one))
        s = _twice(lambda: p.run(entry, grad_scale=big))
        what = f"{name} [{entry}]"
        for u, v in zip(a[:3], b[:3]):
            assert torch.equal(_bits(u.buf), _bits(v.buf)), what + ": grad_scale = 1.0 differs from a null pointer"
        assert torch.equal(_bits(a[0].buf), _bits(s[0].buf)), what + ": grad_scale changed the loss"
        for u, v in zip(a[1:3], s[1:3]):
            g = u.data()
            nz = g[g != 0].abs()
            assert nz.numel() and float(nz.min()) >= 2.0 ** -126 and float(nz.max()) * 65536.0 < 3e38
            assert torch.equal(g * 65536.0, v.data()), what + ": gradients are not exactly 2^16 times the unscaled ones"
