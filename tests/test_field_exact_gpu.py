"""Exact known-answer tests of the fused LiDAR-field kernels the training step runs: lnh_density_mlp_forward / _backward (the
sigma net on level-major features with a strided destination, both feature addressings), the colour head of
csrc/lidar_color.hip (lnh_lidar_color_forward, _composite_forward, _backward, _backward_image, lnh_ragged_color_forward /
_backward) and the direction-term glue (lnh_lidar_dir_term, _backward), fp16 and bf16 builds, through the C ABI.

The problems (tests/field_exact_cases.py) are integer-valued; the gradients that pass a sigmoid or an exponential are
pre-compensated so that the first 16-bit value the backward forms is an exact integer.  Every tensor a kernel writes then has
ONE right value in any summation order and is compared with torch.equal; tests/test_field_exact_cpu.py asserts the conditions.
The discipline is that of tests/test_mlp_exact_gpu.py: sentinel-filled outputs with guard words, 64 NaN rows behind every
floating-point input (and NaN in every row of an input that the kernel has no business reading), weight gradients ADDED to 2.0,
every call made twice with identical bits.

Two outputs are not integers.  sigma = exp(h16[., 0]) keeps the bound of tests/test_lidar_field_gpu.py (rtol 2e-6 against exp
of the exact integer).  rgb = sigmoid(o) is compared with the float64 sigmoid of the exact integer o within a relative
(|o| + 8) 2^-24.  The bound is derived from the kernel's arithmetic, rcp(1 + exp2(-o log2 e)) in fp32, not measured; in units
of 2^-24 (half an fp32 spacing, relative): the product -o log2 e is rounded once (1 unit; the fp32 constant is off by another
0.24), and the exponential turns that relative error of its argument into |o| ln 2 log2 e = |o| times as much in its value;
v_exp_f32 is good to 1 ulp (2 units); all of this reaches rgb scaled by e / (1 + e) <= 1; the sum 1 + e is rounded once
(1 unit) and v_rcp_f32 is good to 1 ulp (2 units).  That is |o| + 5 with the constant taken as exact, and 3 units cover its
0.24 |o| up to |o| = 12; beyond that the term only counts for o < 0 (e / (1 + e) < 2^-17 for o >= 12) and o is an integer, so
the kernel produces one of a few dozen values, all of which the tests below see.
MEASURED on an MI355X, fp16 and bf16 builds alike: the largest deviation over every test of this file is 0.507 of the bound
(dense (2100, 40) and the ragged table; 0.49 in most other shapes) — each test prints its own figure.
"""
import numpy as np
import pytest
import torch

import field_exact_cases as fc
from exact_util import SENT, Out, _dev, _poisoned, _twice

pytestmark = pytest.mark.gpu

DTYPES = {"": torch.float16, "_bf16": torch.bfloat16}
SFX = list(DTYPES)


def _call(name, *args):
    from gpu_util import call
    call(name, *[a.buf if isinstance(a, Out) else a for a in args])


def _ws():
    from gpu_util import wgrad
    return wgrad()


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _i32(a, pad=0):
    """int32 device tensor with `pad` zeros behind it (an index read past the end stays inside the buffers)."""
    t = torch.zeros(a.size + pad, dtype=torch.int32, device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a.reshape(-1), dtype=np.int32)).cuda()
    return t


def _want(a, dt):
    """Expected float64 array (NaN = nobody writes it) -> device tensor with the sentinel in those places."""
    return _dev(np.where(np.isnan(a), SENT, a), dt)


# ================================================================================================ sigma net
class SigmaProblem:
    def __init__(self, shape, sfx):
        self.s = s = fc.get_sigma_case(*shape)
        self.sfx, self.dt, c = sfx, DTYPES[sfx], s.c
        idx = torch.from_numpy(c.idx).cuda()
        self.rows = torch.from_numpy(s.rows).cuda()
        take = lambda a, dt: _dev(a, dt)[idx]
        level_major = lambda t: t.view(s.B, 16, 2).permute(1, 0, 2).contiguous()
        self.feat = level_major(take(c.x, torch.float16))                # [16, B, 2]: fp16 in both builds
        self.w = _dev(c.flat_weights(), self.dt)
        self.want_y, self.want_gfeat = take(c.y, self.dt), level_major(take(c.gx, torch.float16))
        self.gy = take(c.gy, self.dt)
        self.want_dW = torch.cat([_dev(d, torch.float32).reshape(-1) for d in c.dW]) + 2.0
        self.what = f"sigma net (N, T_cur, T_tot, off) = {shape} {'bf16' if sfx else 'fp16'}:"

    def strided(self, t, fill, dt):
        """[B, 16] rows at their destination rows of a [B_all, 16] buffer of `fill`."""
        full = torch.full((self.s.B_all, 16), fill, dtype=dt, device="cuda")
        full[self.rows] = t
        return full

    def forward(self, mapped):
        s = self.s
        if mapped:  # features addressed by the destination row: [16, B_all, 2], NaN in every row that is no destination
            feat = torch.full((16, s.B_all, 2), float("nan"), dtype=torch.float16, device="cuda")
            feat[:, self.rows] = self.feat
        else:
            feat = self.feat
        feat = _poisoned(feat, 32)

        def run():
            h16, sigma = Out((s.B_all, 16), self.dt), Out((s.B_all,), torch.float32)
            _call("lnh_density_mlp_forward" + self.sfx, feat, self.w, s.B, s.T_cur, s.T_tot, s.off, s.B_all if mapped else 0, h16, sigma)
            return h16, sigma
        h16, sigma = _twice(run)
        tag = f"{self.what} forward, feat_rows = {s.B_all if mapped else 0},"
        h16.check(self.strided(self.want_y, SENT, self.dt), f"{tag} h16")
        assert bool((sigma.buf[sigma.n:] == SENT).all()), f"{tag} sigma: guard words overwritten"
        got = sigma.data()
        elsewhere = torch.ones(s.B_all, dtype=torch.bool, device="cuda")
        elsewhere[self.rows] = False
        assert bool((got[elsewhere] == SENT).all()), f"{tag} sigma written outside the destination rows"
        want = torch.exp(self.want_y[:, 0].double())
        torch.testing.assert_close(got[self.rows].double(), want, rtol=2e-6, atol=0.0, msg=lambda m: f"{tag} sigma: {m}")

    def backward(self):
        s = self.s
        gy = _poisoned(self.strided(self.gy, float("nan"), self.dt), 16)
        feat = _poisoned(self.feat, 32)

        def run():
            gfeat, dw = Out((16, s.B, 2), torch.float16), Out((self.w.numel(),), torch.float32, fill=2.0)
            _call("lnh_density_mlp_backward" + self.sfx, gy, feat, self.w, s.B, s.T_cur, s.T_tot, s.off, gfeat, dw, *_ws())
            return gfeat, dw
        gfeat, dw = _twice(run)
        gfeat.check(self.want_gfeat, f"{self.what} backward grad_features")
        dw.check(self.want_dW, f"{self.what} backward dW")


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("shape", fc.SIGMA_SHAPES + [fc.SIGMA_FWD_STRIDE])
def test_sigma_net_forward_both_addressings(shape, sfx):
    """h16 exact at the destination rows and untouched elsewhere, sigma = exp of it, with features indexed by the point
    (feat_rows = 0) and by the destination row (feat_rows = B_all); the last shape is past the forward's first grid-stride
    pass (2048 workgroups x 128 points; periodic rows)."""
    p = SigmaProblem(shape, sfx)
    p.forward(False)
    p.forward(True)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("shape", fc.SIGMA_SHAPES + [fc.SIGMA_FWD_STRIDE, fc.SIGMA_BWD_STRIDE])
def test_sigma_net_backward(shape, sfx):
    """grad_h16 read from the strided rows (NaN in every other row), grad_features exact and level-major, dW exact and added;
    the last shape is past 256 workgroups x 256 points."""
    SigmaProblem(shape, sfx).backward()


# ================================================================================================ colour head
class ColorProblem:
    """A colour problem on the device in one element type.  `tiled`: the periodic forward problem (no backward)."""

    def __init__(self, c, sfx, tiled=None):
        self.c, self.sfx, self.dt = c, sfx, DTYPES[sfx]
        t = (lambda a: tiled.tile(a)) if tiled else (lambda a: a)
        self.N = tiled.N if tiled else c.N
        self.T = c.T
        self.rows = self.N * c.T if tiled else c.rows
        self.h16 = _poisoned(_dev(t(c.x), self.dt), 16)
        self.cdir = _poisoned(_f32(np.concatenate([c.cdir] * tiled.reps)[:self.N] if tiled else c.cdir), 64)
        self.w16 = _dev(c.H.flat(), self.dt)
        if c.ragged:
            self.rays = _i32(c.rays)
        else:
            self.perm = _i32(t(c.perm.reshape(-1)), pad=64)
            self.weights = _poisoned(_f32(t(c.weights)), 1)
        e = c.expected() if not tiled else None
        rgb = t(np.where(c.act[:, None], fc.sigmoid(c.o), 0.0)) if tiled else e["rgb"]
        self.want_rgb = torch.from_numpy(rgb).cuda()                       # float64; NaN = nobody owns the row
        o = np.full((c.rows, 2), np.nan)
        o[c.pos] = np.where(c.act[:, None], c.o, np.nan)
        self.o_abs = torch.from_numpy(np.abs(t(o))).cuda()                # |o| of the active samples
        self.what = f"colour head {'ragged' if c.ragged else (self.N, self.T)} {'bf16' if sfx else 'fp16'}:"
        if not tiled:
            self.g_rgb = _poisoned(_f32(c.g_rgb), 2)
            self.g_sigma = _poisoned(_f32(c.g_sigma), 1)
            self.want_gh = _want(e["g_h16"], self.dt)
            self.want_dW = _dev(c.flat_dW(), torch.float32) + 2.0
            self.want_S = _dev(e["S"], torch.float32)

    def check_rgb(self, rgb, what):
        """0.0 on masked samples, the sentinel on rows nobody owns, sigmoid(o) within (|o| + 8) 2^-24 on active samples."""
        assert bool((rgb.buf[rgb.n:] == SENT).all()), f"{what}: guard words overwritten"
        got, want = rgb.data().double(), self.want_rgb
        unowned, active = torch.isnan(want), ~torch.isnan(self.o_abs)
        assert bool((got[unowned] == SENT).all()), f"{what}: a row nobody owns was written"
        masked = ~unowned & ~active
        assert bool((got[masked] == 0.0).all()), f"{what}: a masked sample is not exactly 0"
        bound = (self.o_abs[active] + fc.RGB_BOUND_ULPS) * 2.0 ** -24 * want[active]
        share = float(((got[active] - want[active]).abs() / bound).max()) if bool(active.any()) else 0.0
        print(f"[rgb] {what} max |rgb - sigmoid(o)| = {share:.3f} of the bound")
        assert share <= 1.0, f"{what}: rgb is off sigmoid(o) by {share:.3f} times (|o| + 8) 2^-24"

    def forward(self):
        c = self.c

        def run():
            rgb = Out((self.rows, 2), torch.float32)
            if c.ragged:
                _call("lnh_ragged_color_forward" + self.sfx, self.h16, self.rays, self.cdir, self.w16, c.N, c.rows, rgb)
            else:
                _call("lnh_lidar_color_forward" + self.sfx, self.h16, self.perm, self.weights, self.cdir, self.w16, self.N, self.T, rgb)
            return (rgb,)
        self.check_rgb(_twice(run)[0], f"{self.what} forward rgb")

    def run_backward(self, entry="rgb", g_rgb=None, g_image=None):
        c = self.c
        g_rgb = self.g_rgb if g_rgb is None else g_rgb
        gh, dw = Out((c.rows, 16), self.dt), Out((self.w16.numel(),), torch.float32, fill=2.0)
        S = Out((c.N, 64), torch.float32)
        if c.ragged:
            _call("lnh_ragged_color_backward" + self.sfx, g_rgb, self.g_sigma, c.scale, self.h16, self.rays, self.cdir, self.w16,
                  c.N, c.rows, gh, dw, S, *_ws())
        elif entry == "rgb":
            _call("lnh_lidar_color_backward" + self.sfx, g_rgb, self.g_sigma, self.h16, self.perm, self.weights, self.cdir,
                  self.w16, c.N, c.T, gh, dw, S, *_ws())
        else:
            _call("lnh_lidar_color_backward_image" + self.sfx, g_image, self.g_sigma, self.h16, self.perm, self.weights,
                  self.cdir, self.w16, c.N, c.T, gh, dw, S, *_ws())
        return gh, dw, S

    def backward(self):
        gh, dw, S = _twice(self.run_backward)
        gh.check(self.want_gh, f"{self.what} backward g_h16")
        dw.check(self.want_dW, f"{self.what} backward dW")
        S.check(self.want_S, f"{self.what} backward S")
        assert bool((dw.data()[64 * 16 + 64 * 64:].view(16, 64)[2:] == 2.0).all())  # (the padded rows of W2)

    def backward_image(self):
        """lnh_lidar_color_backward_image(g_image) == lnh_lidar_color_backward(weights (x) g_image), every output bit for bit."""
        c = self.c
        g = torch.Generator().manual_seed(c.N * 4096 + c.T)
        g_image = torch.randn(c.N, 2, generator=g).cuda()
        w = self.weights[:c.rows].view(c.N, c.T)
        g_rgb = _poisoned((w[..., None] * g_image[:, None, :]).contiguous(), 2)
        g_image = _poisoned(g_image, 2)
        a = _twice(lambda: self.run_backward("rgb", g_rgb=g_rgb))
        b = _twice(lambda: self.run_backward("image", g_image=g_image))
        for u, v, name in zip(a, b, ("g_h16", "dW", "S")):
            v.check(u.data(), f"{self.what} backward_image against backward, {name}")
            assert bool((u.buf[u.n:] == SENT).all())
        assert bool(torch.isfinite(a[0].data().float()).all()) and bool((a[0].data() != SENT).all())


DENSE = fc.COLOR_FWD_SHAPES + fc.COLOR_BWD_SHAPES + fc.COLOR_WAVE_SHAPES


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("N,T", DENSE)
def test_colour_forward(N, T, sfx):
    """k_color_forward: one sample, N T no multiple of 16, whole spans, the span and group shapes of the backward, more rays
    than waves."""
    ColorProblem(fc.get_color_case(N, T), sfx).forward()


@pytest.mark.parametrize("sfx", SFX)
def test_colour_forward_second_grid_stride_pass(sfx):
    """More than 2048 workgroups x 256 samples (a period of 7 rays tiled)."""
    N, T = fc.COLOR_FWD_STRIDE
    t = fc.TiledForward(N, T)
    assert N * T > 2048 * 256
    ColorProblem(t.p, sfx, tiled=t).forward()


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("N,T", DENSE)
def test_colour_backward(N, T, sfx):
    """g_h16 (every row once: column 0 = t' on every sample, columns 1 .. 15 zero off the probes), dW added to 2.0, S with
    every row written (zero for a ray without an active span) — spans of 32 and groups of 1024 samples with a probe as the
    last valid sample of a partial span, as the first of the second group and as the only active sample of a ray; walks of
    several rays per wave with 0 .. 3 active spans, transparent rays first, last and two in a row."""
    ColorProblem(fc.get_color_case(N, T), sfx).backward()


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("N,T", DENSE)
def test_colour_backward_from_image_gradient(N, T, sfx):
    ColorProblem(fc.get_color_case(N, T), sfx).backward_image()


@pytest.mark.parametrize("sfx", SFX)
def test_ragged_colour_forward_and_backward(sfx):
    """The ragged table: ids a permutation of the rows, counts 0 / 1 / 31 / 32 / 33 / 1024 / 1025, a dropped entry, rows
    nobody owns (NaN in every input, the sentinel in every output), density scale 2."""
    p = ColorProblem(fc.get_ragged_case(), sfx)
    p.forward()
    p.backward()


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("T", fc.COMPOSITE_T)
def test_colour_composite_forward(T, sfx):
    """sigma_m exact and rgb by the forward rule, on weights that are exactly 0 or >= 1e-3 in float64 (weights, weights_sum,
    depth and image stay under tests/test_lidar_field_gpu.py)."""
    k = fc.get_composite_case(T)
    p = ColorProblem(k.c, sfx)
    N = k.N
    z, sigma_pt, sd = _poisoned(_f32(k.z), 1), _poisoned(_f32(k.sigma_pt), 1), _poisoned(_f32(k.sd), 1)
    p.want_rgb = torch.from_numpy(k.rgb).cuda()
    p.o_abs = torch.from_numpy(np.where(k.on.reshape(-1, 1), np.abs(k.o), np.nan)).cuda()

    def run():
        outs = [Out(s, torch.float32) for s in ((N, T), (N, T), (N * T, 2), (N,), (N,), (N, 2))]
        _call("lnh_lidar_color_composite_forward" + sfx, z, sigma_pt, p.perm, sd, p.h16, p.cdir, p.w16, N, T, 1.0, *outs)
        return outs
    sigma_m, weights, rgb, wsum, depth, image = _twice(run)
    sigma_m.check(_dev(k.sigma_m, torch.float32), f"{p.what} composite sigma_m")
    p.check_rgb(rgb, f"{p.what} composite rgb")
    for o in (weights, wsum, depth, image):
        assert bool((o.buf[o.n:] == SENT).all()) and bool((o.data() != SENT).all())
    assert torch.equal(weights.data() > fc.THRESH, torch.from_numpy(k.on).cuda())


@pytest.mark.parametrize("sfx", SFX)
def test_colour_composite_forward_refuses_rays_beyond_its_lds(sfx):
    k = fc.get_composite_case(2048)
    p = ColorProblem(k.c, sfx)
    outs = [Out(s, torch.float32) for s in ((1, 2049), (1, 2049), (2049, 2), (1,), (1,), (1, 2))]
    z = _f32(np.zeros(2049))
    with pytest.raises(RuntimeError, match=r"failed \(-2\)"):  # LNH_ERR_UNSUPPORTED
        _call("lnh_lidar_color_composite_forward" + sfx, z, z, _i32(np.zeros(2049)), z, p.h16, p.cdir, p.w16, 1, 2049, 1.0, *outs)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.buf == SENT).all())


# ================================================================================================ direction-term glue
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("K", fc.DIR_K)
def test_dir_term(K, sfx):
    """features16 and cdir exact; the columns of w0 behind K (NaN here) are not read, nothing is written behind an output."""
    for N in fc.DIR_N:
        for ldw in (K + 15, K + 22):
            d = fc.get_dir_case(N, K, ldw)
            f, w0 = _poisoned(_f32(d.f), K), _poisoned(_f32(d.w0), ldw)

            def run():
                f16, cdir = Out((N, K), torch.float32), Out((N, 64), torch.float32)
                _call("lnh_lidar_dir_term" + sfx, f, w0, ldw, N, K, f16, cdir)
                return f16, cdir
            f16, cdir = _twice(run)
            what = f"dir_term{sfx} N {N} K {K} ldw {ldw}:"
            f16.check(_dev(d.f, torch.float32), f"{what} features16")
            cdir.check(_dev(d.cdir, torch.float32), f"{what} cdir")


@pytest.mark.parametrize("K", fc.DIRB_K)
def test_dir_term_backward(K):
    """grad_w0[:, :K] exact and ADDED to 2.0; the packed geo-feature gradient copied to columns K .. K + 14 (its column 0 is
    not), columns beyond K + 15 untouched; without it nothing behind column K is written."""
    for N in fc.DIRB_N:
        for ldw in (K + 15, K + 22):
            d = fc.get_dir_case(N, K, ldw)
            S, f, w0g = _poisoned(_f32(d.S), 64), _poisoned(_f32(d.f), K), _poisoned(_f32(d.w0g), 16)
            for packed in (True, False):
                def run():
                    gw = Out((64, ldw), torch.float32, fill=2.0)
                    _call("lnh_lidar_dir_term_backward", S, f, N, K, w0g if packed else None, gw, ldw, *_ws())
                    return (gw,)
                want = torch.full((64, ldw), 2.0, device="cuda")
                want[:, :K] += _dev(d.gw0, torch.float32)
                if packed:
                    want[:, K:K + 15] = _dev(d.w0g[:, 1:], torch.float32)
                _twice(run)[0].check(want, f"dir_term_backward N {N} K {K} ldw {ldw} packed {packed}: grad_w0")
