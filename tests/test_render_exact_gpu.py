"""Known-answer tests of the per-ray scan kernels the training step runs: lnh_lidar_weights, lnh_lidar_composite_forward /
_backward, lnh_lidar_resample / _strided / _points (csrc/lidar_render.hip), lnh_lidar_merge_weights, lnh_lidar_sample_points and
lnh_lidar_coarse_sample_points (csrc/lidar_field.hip), through the C ABI.

TIER A (tests/render_exact_cases.py; conditions asserted on the CPU by tests/test_render_exact_cpu.py): every sample is
transparent (sigma = 0) or opaque (expf argument <= -1024), depths, colours and gradients lie on dyadic lattices, a ray holds at
most two opaque samples.  Every output then has ONE float32 value in any scan order and is compared with torch.equal: the carries
between 64-sample rounds, between groups of 7 rounds and between the two passes of the backward, the last sample's sample_dist,
the ray of a wave, the colour stride, the row map of the sample positions, both ends of the inverse cdf, the tie rule of the merge.
Discipline of tests/exact_util.py: sentinel-filled outputs with guard words, NaN rows behind every input, every call twice.

TIER B: general alpha against float64 within a bound PER ELEMENT derived from the rounding model (render_exact_cases
forward_bounds / backward_bounds / icdf_reference) — no global tolerance, so the elements far behind the
surface are held as tightly as the peak.  Each test prints the largest error / bound it sees; it must not exceed 1.
MEASURED on an MI355X (E = 1.68), largest error / bound: weights 0.185, weights_sum / depth / image 0.009, g_sigma 0.109, g_rgb 0.185,
inverse cdf 0.246 on the steep-bin rays and 0.077 on smooth rays.
"""

import numpy as np
import pytest
import torch

import render_exact_cases as rc
from exact_util import SENT, Out, _poisoned, _twice

pytestmark = pytest.mark.gpu
F = np.float32


def _call(name, *args):
    from gpu_util import call
    call(name, *[a.buf if isinstance(a, Out) else a for a in args])


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _i32(a, pad=64):
    t = torch.zeros(a.size + pad, dtype=torch.int32, device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a.reshape(-1), dtype=np.int32)).cuda()
    return t


def _nan_out(shape):
    return Out(shape, torch.float32, fill=float("nan"))


def _check_nan_rows(out, want, what):
    """`want` holds NaN where nobody may write: those words must still hold their NaN, the rest must match bit for bit."""
    assert bool((out.buf[out.n:] == SENT).all()), f"{what}: guard words behind the buffer were overwritten"
    got, want = out.data(), _f32(want).view(out.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: a row outside the map was written (or one inside was not)"
    assert torch.equal(torch.nan_to_num(got, nan=SENT), torch.nan_to_num(want, nan=SENT)), f"{what}: values differ"


# ================================================================================================ tier A: compositing
class Composite:
    def __init__(self, shape):
        self.c = c = rc.get_composite_case(*shape)
        self.N, self.T, self.K = c.N, c.T, c.K
        self.z, self.sigma = _poisoned(_f32(c.z), c.T), _poisoned(_f32(c.sigma), c.T)
        self.rgb, self.sd = _poisoned(_f32(c.rgb), c.T * c.K), _poisoned(_f32(c.sd), 1)
        self.g = {"g_ws": _poisoned(_f32(c.g_ws), 1), "g_depth": _poisoned(_f32(c.g_depth), 1),
                  "g_image": _poisoned(_f32(c.g_image), c.K)}
        self.what = f"(N, T, K, scale, first) = {shape}:"


SHAPES = rc.composite_shapes()


@pytest.mark.parametrize("shape", SHAPES)
def test_weights(shape):
    p = Composite(shape)
    want = _f32(p.c.expected()["weights"])

    def run():
        w = Out((p.N, p.T), torch.float32)
        _call("lnh_lidar_weights", p.z, p.sigma, p.sd, p.N, p.T, p.c.ds, w)
        return (w,)
    _twice(run)[0].check(want, f"{p.what} lnh_lidar_weights")


@pytest.mark.parametrize("with_weights", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_composite_forward(shape, with_weights):
    p = Composite(shape)
    e = p.c.expected()

    def run():
        w = Out((p.N, p.T), torch.float32)
        ws, dep, img = Out((p.N,), torch.float32), Out((p.N,), torch.float32), Out((p.N, p.K), torch.float32)
        _call("lnh_lidar_composite_forward", p.z, p.sigma, p.rgb, p.sd, p.N, p.T, p.K, p.c.ds, w if with_weights else None, ws, dep, img)
        return w, ws, dep, img
    w, ws, dep, img = _twice(run)
    w.check(_f32(e["weights"]) if with_weights else torch.full((p.N, p.T), SENT, device="cuda"), f"{p.what} forward weights")
    ws.check(_f32(e["weights_sum"]), f"{p.what} forward weights_sum")
    dep.check(_f32(e["depth"]), f"{p.what} forward depth")
    img.check(_f32(e["image"]), f"{p.what} forward image")


@pytest.mark.parametrize("variant", ["all", "g_ws", "g_depth", "g_image", "no grad_rgb"])
@pytest.mark.parametrize("shape", SHAPES)
def test_composite_backward(shape, variant):
    """All gradients given; g_ws, g_depth, g_image null in turn; grad_rgb = NULL.  g_sigma is compared on the rays with at most
    one opaque sample (with two, the suffix of the first is a cancelled difference), g_rgb on every ray."""
    p = Composite(shape)
    null = (variant,) if variant.startswith("g_") else ()
    e = p.c.expected(null)
    g = {k: (None if k in null else v) for k, v in p.g.items()}

    def run():
        gs, gc = Out((p.N, p.T), torch.float32), Out((p.N, p.T, p.K), torch.float32)
        _call("lnh_lidar_composite_backward", g["g_ws"], g["g_depth"], g["g_image"], p.z, p.sigma, p.rgb, p.sd, p.N, p.T, p.K,
              p.c.ds, gs, None if variant == "no grad_rgb" else gc)
        return gs, gc
    gs, gc = _twice(run)
    want = _f32(np.nan_to_num(e["g_sigma"], nan=0.0))
    skip = torch.from_numpy(np.isnan(e["g_sigma"])).cuda()
    assert bool((gs.data()[skip] != SENT).all())
    gs.check(torch.where(skip, gs.data(), want), f"{p.what} backward ({variant}) g_sigma")
    gc.check(torch.full((p.N, p.T, p.K), SENT, device="cuda") if variant == "no grad_rgb" else _f32(e["g_rgb"]),
             f"{p.what} backward ({variant}) g_rgb")


@pytest.mark.parametrize("shape", SHAPES)
def test_merge_weights(shape):
    """sigma_pt in point order behind a random permutation per ray: sigma_m the exact gather, weights the closed form."""
    p = Composite(shape)
    e = p.c.expected()
    sigma_pt, perm = _poisoned(_f32(p.c.sigma_pt), p.T), _i32(p.c.perm)

    def run():
        sm, w = Out((p.N, p.T), torch.float32), Out((p.N, p.T), torch.float32)
        _call("lnh_lidar_merge_weights", p.z, sigma_pt, perm, p.sd, p.N, p.T, p.c.ds, sm, w)
        return sm, w
    sm, w = _twice(run)
    sm.check(_f32(e["sigma_m"]), f"{p.what} merge sigma_m")
    w.check(_f32(e["weights"]), f"{p.what} merge weights")


def test_merge_weights_of_no_samples_writes_nothing():
    p = Composite(SHAPES[0])
    sm, w = Out((8,), torch.float32), Out((8,), torch.float32)
    _call("lnh_lidar_merge_weights", p.z, p.sigma, _i32(p.c.perm), p.sd, p.N, 0, 1.0, sm, w)
    torch.cuda.synchronize()
    assert bool((sm.buf == SENT).all()) and bool((w.buf == SENT).all())


# ================================================================================================ tier A: sample positions
@pytest.mark.parametrize("bound", [1.0, 2.0])
@pytest.mark.parametrize("N,T", rc.POINT_SHAPES)
def test_sample_points_row_map(N, T, bound):
    p = rc.PointsCase(N, T, bound)
    o, d, z, aabb = _poisoned(_f32(p.o), 3), _poisoned(_f32(p.d), 3), _poisoned(_f32(p.z), T), _f32(p.aabb)
    T_tot = T + 9
    for slot_off in (0, 5, T_tot - T):
        def run():
            x = _nan_out((N * T_tot, 3))
            _call("lnh_lidar_sample_points", o, d, z, aabb, bound, N, T, T_tot, slot_off, x)
            return (x,)
        _check_nan_rows(_twice(run)[0], p.rows(T_tot, slot_off).reshape(-1, 3), f"sample_points {(N, T, bound)} slot_off {slot_off}")
    with pytest.raises(RuntimeError, match="slot_off"):
        _call("lnh_lidar_sample_points", o, d, z, aabb, bound, N, T, T_tot, 10, _nan_out((N * T_tot, 3)))


@pytest.mark.parametrize("bound", [1.0, 2.0])
@pytest.mark.parametrize("N,T", rc.COARSE_SHAPES)
def test_coarse_sample_points(N, T, bound):
    """Depths and grid coordinates against the float32 restatement of csrc/lidar_steps.h (exact arithmetic where T - 1 is a power
    of two: tests/test_render_exact_cpu.py), without noise, with u = 0.5 (the same bits) and with random noise."""
    p = rc.PointsCase(N, T, bound)
    near, far, T_tot = 0.25, 2.25, T + 3
    o, d, aabb = _poisoned(_f32(p.o), 3), _poisoned(_f32(p.d), 3), _f32(p.aabb)
    noise = np.random.default_rng(N * 1000 + T).random((N, T)).astype(F)
    for name, u in (("no noise", None), ("u = 0.5", np.full((N, T), 0.5, F)), ("noise", noise)):
        ud = None if u is None else _poisoned(_f32(u), T)

        def run():
            z, x = Out((N, T), torch.float32), _nan_out((N * T_tot, 3))
            _call("lnh_lidar_coarse_sample_points", ud, o, d, aabb, bound, N, T, T_tot, near, far, z, x)
            return z, x
        z, x = _twice(run)
        t = rc.coarse_depths_f32(N, T, near, far, u)
        if name == "u = 0.5":
            assert np.array_equal(t, rc.coarse_depths_f32(N, T, near, far, None))
        z.check(_f32(t), f"coarse {(N, T, bound)} {name}: z")
        rows = np.full((N, T_tot, 3), np.nan, F)
        rows[:, :T] = rc.sample_points_f32(p.o, p.d, t, p.aabb, bound)
        _check_nan_rows(x, rows.reshape(-1, 3), f"coarse {(N, T, bound)} {name}: x01")


# ================================================================================================ tier A: resampling
def _resample(c, entry, sorted_new):
    N, T, n = c.N, c.T, c.n
    z, sd, u = _poisoned(_f32(c.z), T), _poisoned(_f32(c.sd), 1), _poisoned(_f32(c.u), n)
    wide = np.full((N, T + n), np.nan, F)
    wide[:, :T] = c.sigma
    sigma = _poisoned(_f32(c.sigma), T) if entry == "lnh_lidar_resample" else _poisoned(_f32(wide), T + n)
    o, d, aabb = _poisoned(_f32(c.o), 3), _poisoned(_f32(c.d), 3), _f32(c.aabb)

    def run():
        new_z, z_out = Out((N, n), torch.float32), Out((N, T + n), torch.float32)
        perm = Out((N, T + n), torch.int32)
        if entry == "lnh_lidar_resample":
            _call(entry, z, sigma, sd, u, N, T, n, 1.0, sorted_new, new_z, z_out, perm)
            return new_z, z_out, perm
        if entry == "lnh_lidar_resample_strided":
            _call(entry, z, sigma, T + n, sd, u, N, T, n, 1.0, sorted_new, new_z, z_out, perm)
            return new_z, z_out, perm
        x = _nan_out((N * (T + n), 3))
        _call(entry, z, sigma, T + n, sd, u, N, T, n, 1.0, new_z, z_out, perm, o, d, aabb, c.bound, x)
        return new_z, z_out, perm, x
    return _twice_i(run)


def _twice_i(fn):
    """_twice for outputs that include an int32 buffer."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert torch.equal(u.buf.view(torch.int32), v.buf.view(torch.int32)), "two identical calls gave different bits"
    return a


@pytest.mark.parametrize("shape", rc.RESAMPLE_SHAPES)
def test_resample_ends_and_merge_order(shape):
    """u = 0 -> z_mid[0] and u = 1.0 -> z_mid[T-2] exactly (several j each); every sample of a ray with T <= 4, one u on cdf[1];
    perm = the stable sort of concat([old, new]) with z_0 = z_1 = z_mid[0] = several new keys; sorted_new = 1: slot T + r holds the
    r-th smallest key; the x01 rows of lnh_lidar_resample_points; n_new around the padded lengths; the call above 64 KiB of LDS."""
    c = rc.get_resample_case(*shape)
    N, T, n = shape
    zm = c.z_mid().astype(F)
    new_z, z_out, perm = _resample(c, "lnh_lidar_resample", 0)
    for o in (new_z, z_out, perm):
        assert bool((o.buf[o.n:] == SENT).all()), "guard words overwritten"
    got = new_z.data().cpu().numpy()
    assert np.array_equal(got[c.at0], np.broadcast_to(zm[:, :1], got.shape)[c.at0]), "u = 0 must give z_mid[0] exactly"
    assert np.array_equal(got[c.at1], np.broadcast_to(zm[:, -1:], got.shape)[c.at1]), "u = 1.0 must give z_mid[T-2] exactly"
    if T <= 4:
        want = np.stack([rc.icdf_small(c.z[r], c.sigma[r], c.sd[r], c.u[r]) for r in range(N)])
        assert np.array_equal(got, want), "inverse cdf of the small rays"
    assert np.all(got >= zm[:, :1]) and np.all(got <= zm[:, -1:])
    ref0 = [rc.merge_reference(c.z[r], got[r], 0) for r in range(N)]
    z_out.check(_f32(np.stack([m[0] for m in ref0])), f"resample {shape}: z_out")
    perm.check(torch.from_numpy(np.stack([m[1] for m in ref0])).cuda(), f"resample {shape}: perm = stable sort, old first")
    ref1 = [rc.merge_reference(c.z[r], got[r], 1) for r in range(N)]
    want1 = (_f32(np.stack([m[2] for m in ref1])), _f32(np.stack([m[0] for m in ref1])),
             torch.from_numpy(np.stack([m[1] for m in ref1])).cuda())
    for entry in ("lnh_lidar_resample", "lnh_lidar_resample_strided", "lnh_lidar_resample_points"):
        outs = _resample(c, entry, 1)
        for o, w, name in zip(outs, want1, ("new_z", "z_out", "perm")):
            o.check(w, f"{entry} {shape} sorted_new = 1: {name}")
        if entry == "lnh_lidar_resample_points":
            rows = np.full((N, T + n, 3), np.nan, F)
            rows[:, T:] = rc.sample_points_f32(c.o, c.d, np.stack([m[2] for m in ref1]), c.aabb, c.bound)
            _check_nan_rows(outs[3], rows.reshape(-1, 3), f"{entry} {shape}: x01")


@pytest.mark.parametrize("N,T,n_new", rc.RESAMPLE_REFUSED)
def test_resample_refusals(N, T, n_new):
    """T = 2, n_new = 0 and 1025, and a ray above 160 KiB of LDS: refused, nothing written."""
    z = torch.zeros(N * max(T, 3), device="cuda")
    outs = [Out((N, max(n_new, 1)), torch.float32), Out((N, T + n_new), torch.float32), Out((N, T + n_new), torch.int32)]
    with pytest.raises(RuntimeError, match="lidar_resample"):
        _call("lnh_lidar_resample", z, z, z, z, N, T, n_new, 1.0, 0, *outs)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.buf == SENT).all())


# ================================================================================================ tier B
def _utilisation(got, want, bound, what, skip=None):
    """Largest |got - want| / bound over the elements with a finite bound; a bound of 0 asks for the exact value."""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    use = np.isfinite(bound) if skip is None else np.isfinite(bound) & ~skip
    assert use.mean() > 0.98, f"{what}: {1 - use.mean():.4f} of the elements left out"
    err = np.abs(got - want)
    zero = use & (bound == 0)
    assert np.all(err[zero] == 0), f"{what}: {int((err[zero] != 0).sum())} elements with an exact answer are off"
    use &= bound > 0
    share = float((err[use] / bound[use]).max())
    at = np.unravel_index(np.argmax(np.where(use, err / np.where(use, bound, 1.0), 0.0)), err.shape)
    print(f"[bound] {what}: max error / bound = {share:.3f} at {tuple(int(i) for i in at)} ({int(use.sum())} elements, {int((~np.isfinite(bound)).sum())} skipped)")
    assert share <= 1.0, f"{what}: off by {share:.3f} times the derived bound at {at}: got {got[at]!r}, want {want[at]!r}"
    return share


def _forward_case(name):
    if name == "old profile":
        z, sigma, rgb, sd = rc._old_profile(37, 832, 1)
        return z, sigma, rgb, sd
    return rc.two_surface_rays()[:4]


@pytest.mark.parametrize("name", ["old profile", "two surfaces"])
def test_forward_within_the_derived_bounds(name):
    z, sigma, rgb, sd = _forward_case(name)
    N, T, K = rgb.shape
    fb = rc.forward_bounds(z, sigma, sd, 1.0)
    zc, sc, cc, sdc = _f32(z), _f32(sigma), _f32(rgb), _f32(sd)
    w = Out((N, T), torch.float32)
    _call("lnh_lidar_weights", zc, sc, sdc, N, T, 1.0, w)
    _utilisation(w.data().cpu().numpy(), fb["w"], fb["d_w"], f"lnh_lidar_weights, {name}")
    w2, ws, dep, img = Out((N, T), torch.float32), Out((N,), torch.float32), Out((N,), torch.float32), Out((N, K), torch.float32)
    _call("lnh_lidar_composite_forward", zc, sc, cc, sdc, N, T, K, 1.0, w2, ws, dep, img)
    assert torch.equal(w2.data(), w.data())
    z64, rgb64 = z.astype(np.float64), rgb.astype(np.float64)
    one = np.ones_like(z64)
    _utilisation(ws.data().cpu().numpy(), fb["w"].sum(1), rc.sum_bounds(fb["w"], fb["d_w"], one), f"weights_sum, {name}")
    _utilisation(dep.data().cpu().numpy(), (fb["w"] * z64).sum(1), rc.sum_bounds(fb["w"], fb["d_w"], z64), f"depth, {name}")
    bound = np.stack([rc.sum_bounds(fb["w"], fb["d_w"], rgb64[..., k]) for k in range(K)], axis=1)
    _utilisation(img.data().cpu().numpy(), (fb["w"][..., None] * rgb64).sum(1), bound, f"image, {name}")
    # merge_weights with the identity permutation runs the same scan
    sm, w3 = Out((N, T), torch.float32), Out((N, T), torch.float32)
    _call("lnh_lidar_merge_weights", zc, sc, _i32(np.tile(np.arange(T), (N, 1))), sdc, N, T, 1.0, sm, w3)
    _utilisation(w3.data().cpu().numpy(), fb["w"], fb["d_w"], f"lnh_lidar_merge_weights, {name}")


@pytest.mark.parametrize("case", ["two surfaces", 1, 2, 3, 4])
def test_backward_within_the_derived_bounds(case):
    """g_sigma and g_rgb against float64 (= autograd of the oracle, tests/test_render_exact_cpu.py) element by element; K = 1 .. 4 on
    the profile of test_composite_backward_matches_autograd WITHOUT its clamp: the opaque ray runs backward."""
    z, sigma, rgb, sd, gws, gdp, gim = rc.two_surface_rays() if case == "two surfaces" else rc.old_profile_backward(case)
    N, T, K = rgb.shape
    b = rc.backward_bounds(z, sigma, rgb, sd, 1.0, gws, gdp, gim)
    gs, gc = Out((N, T), torch.float32), Out((N, T, K), torch.float32)
    _call("lnh_lidar_composite_backward", _f32(gws), _f32(gdp), _f32(gim), _f32(z), _f32(sigma), _f32(rgb), _f32(sd), N, T, K, 1.0, gs, gc)
    got = gs.data().cpu().numpy()
    assert np.isfinite(got).all()
    _utilisation(got, b["g_sigma"], b["d_g_sigma"], f"g_sigma, {case}")
    _utilisation(gc.data().cpu().numpy(), b["g_rgb"], b["d_g_rgb"], f"g_rgb, {case}")


@pytest.mark.parametrize("case", rc.ICDF_CASES)
def test_inverse_cdf_within_the_derived_bounds(case):
    z, sigma, sd, u = rc.icdf_inputs(case)
    N, T = z.shape
    n = u.shape[1]
    ref = rc.icdf_reference(z, sigma, sd, 1.0, u)
    new_z, z_out, perm = Out((N, n), torch.float32), Out((N, T + n), torch.float32), Out((N, T + n), torch.int32)
    _call("lnh_lidar_resample", _f32(z), _f32(sigma), _f32(sd), _f32(u), N, T, n, 1.0, 0, new_z, z_out, perm)
    _utilisation(new_z.data().cpu().numpy(), ref["s"], ref["bound"], f"inverse cdf, {case}", skip=ref["excluded"])
