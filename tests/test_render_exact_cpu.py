"""The problems of tests/test_render_exact_gpu.py, checked without a GPU: the conditions that make a bit-for-bit comparison of the
per-ray compositing / resampling kernels meaningful (tests/render_exact_cases.py: lattices, powers of two, at most two opaque
samples, -ffp-contract=off), the closed forms against the float64 oracle and autograd, coverage of every position class, the
teeth of the derived tier-B bounds, the shares they leave out, and the sensitivity of the reference to each classic mistake."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import render_exact_cases as rc
from oracle import render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_library_is_built_without_fp_contraction():
    """The closed forms and the float32 restatements count one rounding per operation."""
    spec = importlib.util.spec_from_file_location("lnh_build", os.path.join(ROOT, "lidar-nerf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "-ffp-contract=off" in mod.FLAGS and not any("fast-math" in f for f in mod.FLAGS)


def _oracle64(c, null=()):
    """Weights, sums and autograd gradients of the float64 oracle on a tier-A problem."""
    z = torch.from_numpy(c.z)
    sg = torch.from_numpy(c.sigma).requires_grad_(True)
    cg = torch.from_numpy(c.rgb).requires_grad_(True)
    if c.T > 1:
        w, _ = render_ref.weights_from_sigma(z, sg, torch.from_numpy(c.sd)[:, None], c.ds)
    else:                                                        # (the oracle takes the shape of its last delta from z[1:] - z[:-1])
        w = 1 - torch.exp(-torch.from_numpy(c.sd)[:, None] * c.ds * sg)
    ws, dep, img = w.sum(-1), (w * z).sum(-1), (w[..., None] * cg).sum(-2)
    g = {k: torch.from_numpy(0 * v if k in null else v) for k, v in (("g_ws", c.g_ws), ("g_depth", c.g_depth), ("g_image", c.g_image))}
    ((ws * g["g_ws"]).sum() + (dep * g["g_depth"]).sum() + (img * g["g_image"]).sum()).backward()
    return {"weights": w.detach().numpy(), "weights_sum": ws.detach().numpy(), "depth": dep.detach().numpy(),
            "image": img.detach().numpy(), "g_sigma": sg.grad.numpy(), "g_rgb": cg.grad.numpy()}


@pytest.mark.parametrize("shape", rc.composite_shapes())
def test_composite_problems(shape):
    c = rc.get_composite_case(*shape)                           # (asserts check_conditions)
    for null in ((), ("g_ws",), ("g_depth",), ("g_image",)):
        e, m = c.expected(null), rc.simulate(c, null=null)
        cmp = ~np.isnan(e["g_sigma"])
        assert np.array_equal(cmp.all(1), c.n_opaque <= 1)
        for k in ("weights", "weights_sum", "depth", "image", "g_rgb", "sigma_m"):   # closed forms == the structural model
            assert np.array_equal(e[k], m[k]), k
        assert np.array_equal(e["g_sigma"][cmp].astype(F), m["g_sigma"][cmp])
        assert np.array_equal(e["g_sigma"][cmp].astype(F).astype(np.float64), e["g_sigma"][cmp])
        o = _oracle64(c, null)                                   # closed forms == float64 oracle and autograd
        for k in ("weights", "weights_sum", "depth", "image", "g_rgb"):
            # (rtol: the oracle's own (1 + 1e-15)^i in front of a transparent stretch, 5e-13 at i = 448)
            np.testing.assert_allclose(e[k].astype(np.float64), o[k], rtol=1e-12, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(e["g_sigma"][cmp], o["g_sigma"][cmp], rtol=1e-12, atol=1e-12)
        for r in np.flatnonzero(c.n_opaque == 1):               # behind the surface the values are ~1e-15: relative there
            np.testing.assert_allclose(e["g_sigma"][r, c.i0[r] + 1:], o["g_sigma"][r, c.i0[r] + 1:], rtol=3e-7, atol=0)
            np.testing.assert_allclose(e["weights"][r].astype(np.float64), o["weights"][r], rtol=1e-7, atol=0)
    assert np.array_equal(rc.simulate(c, merge=True)["weights"], c.expected()["weights"])


def test_every_position_class_is_met():
    met = rc.coverage()
    assert met["T"] == set(rc.T_SET) and met["N"] == set(rc.N_SET) and met["K"] == set(rc.K_SET) and met["ds"] == {1.0, 2.0}
    assert met["i0"] == set(rc.I0_SET) | {"T-1"}
    assert met["i1"] == {"same round", "next round", "next group"}
    assert met["flags"] == {"no opaque sample", "sample_dist = 0", "rgb[i0] = 0 with a second opaque sample",
                            "z[i0] = 0 with a second opaque sample"}
    for K in rc.K_SET:                                           # every K sees rays of every count class, both directions
        cases = [rc.get_composite_case(*s) for s in rc.composite_shapes() if s[2] == K]
        assert {int(n) for c in cases for n in c.n_opaque} == {0, 1, 2}
    for shape in rc.composite_shapes():                          # the opaque sample at T - 1 is opaque through sample_dist alone
        c = rc.get_composite_case(*shape)
        for r, i0 in enumerate(c.i0):
            if i0 == c.T - 1:
                assert c.sd[r] > 0 and c.expected()["weights"][r, i0] == 1.0


def test_broken_problems_are_rejected():
    c = rc.CompositeCase(9, 449, 2, 1, 0)
    c.check_conditions()
    r = int(np.flatnonzero(c.n_opaque == 2)[0])
    c.sigma[r, c.i1[r] + 3] = rc.OPAQUE                          # a third opaque sample
    c.n_opaque[r] = 3
    with pytest.raises(AssertionError, match="denormal"):
        c.check_conditions()
    c = rc.CompositeCase(9, 449, 2, 1, 0)
    c.z[0, 5] += 2.0 ** -12
    with pytest.raises(AssertionError):
        c.check_conditions()
    c = rc.CompositeCase(9, 449, 2, 1, 0)
    c.sigma[c.sigma > 0] = 2.0 ** 16                             # expf(-64) is not the same on every implementation
    with pytest.raises(AssertionError):
        c.check_conditions()


# ------------------------------------------------------------------------------------------------ sample positions
def test_sample_point_problems():
    assert {N * T for N, T in rc.POINT_SHAPES} >= {1, 255, 256, 257}
    for bound in (1.0, 2.0):
        lo, hi = rc.AABBS[bound][:3], rc.AABBS[bound][3:]
        assert np.all(np.abs(lo) <= bound) and np.all(np.abs(hi) <= bound)
        sides = set()
        for N, T in rc.POINT_SHAPES:
            p = rc.PointsCase(N, T, bound)
            x = p.x01()                                          # (asserts float32 exactness)
            assert np.array_equal(rc.sample_points_f32(p.o, p.d, p.z, p.aabb, bound).astype(np.float64), x)
            raw = p.o[:, None, :] + p.d[:, None, :] * p.z[..., None]
            sides |= {k for k, m in (("below", raw < lo), ("above", raw > hi), ("inside", (raw > lo) & (raw < hi))) if m.any()}
            assert x.min() >= 0.0 and x.max() <= 1.0
        assert sides == {"below", "above", "inside"}
    assert rc.AABBS[2.0][0] != -rc.AABBS[2.0][3]


def test_coarse_depths_are_exact_where_the_step_is_a_power_of_two():
    near, far = 0.25, 2.25
    for T in rc.COARSE_T:
        assert (T - 1) & (T - 2) == 0
        want = near + (far - near) * np.arange(T) / (T - 1)
        for u in (None, np.full((3, T), 0.5, F)):
            assert np.array_equal(rc.coarse_depths_f32(3, T, near, far, u).astype(np.float64), np.broadcast_to(want, (3, T)))
    assert {T for _, T in rc.COARSE_SHAPES} >= set(rc.COARSE_T) and {N * T for N, T in rc.COARSE_SHAPES} >= {1, 255, 256, 257}


# ------------------------------------------------------------------------------------------------ resampling
def test_resample_problems():
    assert {n for _, _, n in rc.RESAMPLE_SHAPES} == {1, 7, 63, 64, 65, 128, 1024}
    assert [rc.padded(n) for n in (1, 7, 63, 64, 65, 128, 1024)] == [64, 64, 64, 64, 128, 128, 1024]
    assert {T for _, T, _ in rc.RESAMPLE_SHAPES} == {3, 4, 65, 66, 768, 8200}
    assert (2, 8200, 64) in rc.RESAMPLE_SHAPES and rc.resample_lds_bytes(8200, 64) > 64 * 1024
    assert all(rc.resample_lds_bytes(T, n) <= 160 * 1024 for _, T, n in rc.RESAMPLE_SHAPES)
    assert [(T, n) for _, T, n in rc.RESAMPLE_REFUSED[:3]] == [(2, 64), (768, 0), (768, 1025)]
    assert rc.resample_lds_bytes(*rc.RESAMPLE_REFUSED[3][1:]) > 160 * 1024
    for shape in rc.RESAMPLE_SHAPES:
        c = rc.get_resample_case(*shape)                         # (asserts check_conditions)
        assert (c.u[c.at0] == 0).all() and (c.u[c.at1] == 1).all() and c.u.min() >= 0 and c.u.max() <= 1
        zm = c.z_mid()
        # nearly all mass in the last bin: t = 1 - O(U) lands on z_mid[T-2] even if the float32 cdf ends an ulp above 1
        ref = rc.icdf_reference(c.z.astype(F), c.sigma.astype(F), c.sd.astype(F), 1.0, c.u)
        mass = ref["cdf"][:, -1] - ref["cdf"][:, -2]
        assert np.all(mass > 0.9)
        if c.T > 3:                                              # (T = 3: one pdf term, the cdf is [0, 1] exactly)
            width = zm[:, -1] - zm[:, -2]
            assert np.all(ref["d_cdf"][:, -1] / mass * width < 0.5 * np.spacing(zm[:, -1].astype(F)))
        assert np.array_equal(ref["s"][c.at0], np.broadcast_to(zm[:, :1], c.u.shape)[c.at0])
        np.testing.assert_allclose(ref["s"][c.at1], np.broadcast_to(zm[:, -1:], c.u.shape)[c.at1], rtol=1e-12)
        if c.T <= 4:                                             # the float32 restatement of the small rays, vs float64
            for r in range(c.N):
                s32 = rc.icdf_small(c.z[r], c.sigma[r], c.sd[r], c.u[r])
                knot = c.u[r] == rc.small_cdf(c.z[r], c.sigma[r], c.sd[r])[1]   # (float64 has that knot an ulp elsewhere)
                np.testing.assert_allclose(s32[~knot], ref["s"][r][~knot], rtol=0, atol=1e-7)
                assert c.T != 4 or c.n < 7 or (knot.sum() == 1 and s32[knot][0] == zm[r, 1].astype(F))
                assert np.array_equal(s32[c.at0[r]], np.full(c.at0[r].sum(), zm[r, 0], F))
                assert np.array_equal(s32[c.at1[r]], np.full(c.at1[r].sum(), zm[r, -1], F))


def test_merge_reference_is_the_stable_sort():
    c = rc.get_resample_case(5, 4, 7)
    for r in range(c.N):
        new_z = rc.icdf_small(c.z[r], c.sigma[r], c.sd[r], c.u[r])
        assert (new_z == F(c.z[r, 0])).sum() >= 2 and c.z[r, 0] == c.z[r, 1]       # old-old, old-new and new-new ties
        cat = torch.cat([torch.from_numpy(c.z[r].astype(F)), torch.from_numpy(new_z)])
        zs, idx = torch.sort(cat, stable=True)
        z_out, perm, _ = rc.merge_reference(c.z[r], new_z, 0)
        assert np.array_equal(z_out, zs.numpy()) and np.array_equal(perm, idx.numpy().astype(np.int32))
        z_out1, perm1, nz1 = rc.merge_reference(c.z[r], new_z, 1)
        assert np.array_equal(z_out1, z_out) and np.array_equal(nz1, np.sort(new_z))
        assert np.array_equal(np.concatenate([c.z[r].astype(F), nz1])[perm1], z_out)
        assert np.array_equal(perm1[perm1 >= c.T], c.T + np.arange(c.n))             # slot T + r holds the r-th smallest key


# ------------------------------------------------------------------------------------------------ tier B
def test_backward_bound_has_teeth():
    """Dropping w_j c_j from the suffix of sample i moves the float64 g_sigma_i by more than twice its bound: inside a round,
    across a round, across a group, and with i well behind the first surface."""
    z, sigma, rgb, sd, gws, gdp, gim = rc.two_surface_rays()
    b = rc.backward_bounds(z, sigma, rgb, sd, 1.0, gws, gdp, gim)
    assert np.isfinite(b["d_g_sigma"]).all()
    kinds = set()
    for r, i, j in rc.TEETH_PAIRS:
        d = rc.backward_bounds(z, sigma, rgb, sd, 1.0, gws, gdp, gim, drop=(r, i, j))
        moved = abs(d["g_sigma"][r, i] - b["g_sigma"][r, i])
        assert moved > 2 * b["d_g_sigma"][r, i], (r, i, j, moved / b["d_g_sigma"][r, i])
        kinds.add("group" if j // rc.GROUP > i // rc.GROUP else "round" if j // rc.ROUND > i // rc.ROUND else "inside")
        if i == 300:
            assert b["fb"]["w"][r, 190:215].sum() > 0.2 and b["fb"]["w"][r, i] < 1e-2 * b["fb"]["w"][r].max()
            kinds.add("behind")
    assert kinds == {"inside", "round", "group", "behind"}
    # the float64 reference of the bounds is autograd of the oracle
    sg, cg, zt = torch.from_numpy(sigma).double().requires_grad_(True), torch.from_numpy(rgb).double().requires_grad_(True), torch.from_numpy(z).double()
    w, _ = render_ref.weights_from_sigma(zt, sg, torch.from_numpy(sd).double()[:, None])
    ((w.sum(-1) * torch.from_numpy(gws).double()).sum() + ((w * zt).sum(-1) * torch.from_numpy(gdp).double()).sum()
     + ((w[..., None] * cg).sum(-2) * torch.from_numpy(gim).double()).sum()).backward()
    np.testing.assert_allclose(b["g_sigma"], sg.grad.numpy(), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(b["g_rgb"], cg.grad.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("K", rc.K_SET)
def test_skipped_share_of_the_opaque_ray_profile(K):
    z, sigma, rgb, sd, gws, gdp, gim = rc.old_profile_backward(K)
    assert sigma[1].min() == 1e6 and sigma.max() > 2000.0       # unclamped
    b = rc.backward_bounds(z, sigma, rgb, sd, 1.0, gws, gdp, gim)
    assert not np.isnan(b["d_g_sigma"]).any() and not np.isnan(b["d_g_rgb"]).any()
    assert (~np.isfinite(b["d_g_sigma"])).mean() < 0.01 and (~np.isfinite(b["fb"]["d_w"])).mean() < 0.01
    assert (b["d_g_sigma"][1] == 0).sum() > 400                 # the opaque ray is compared: exact zeros where e = 0


@pytest.mark.parametrize("case", rc.ICDF_CASES)
def test_excluded_share_of_the_inverse_cdf(case):
    z, sigma, sd, u = rc.icdf_inputs(case)
    ref = rc.icdf_reference(z, sigma, sd, 1.0, u)
    assert ref["excluded"].mean() < 0.02 and np.isfinite(ref["bound"][~ref["excluded"]]).all()
    if case == "steep":
        _, _, _, _, i0s = rc.steep_rays()
        assert i0s == (1, 62, 63, 64, 65, rc.STEEP_T - 2) and not ref["excluded"].any()
        cdf = ref["cdf"]
        lo = np.stack([np.searchsorted(cdf[r], u[r].astype(np.float64), side="right") for r in range(len(i0s))])
        for r, i0 in enumerate(i0s):
            inside = lo[r] - 1 == i0 - 1
            assert inside.any() and (i0 == 1 or (~inside).any())
            denom = cdf[r, np.minimum(lo[r], rc.STEEP_T - 2)] - cdf[r, lo[r] - 1]
            assert np.all(denom[~inside] < 0.995e-5) and np.all(denom[inside] > 0.9)   # the branch, far from its threshold
        assert ref["bound"].max() < 1e-2 * 2.0 ** -11            # a hundredth of a bin


# ------------------------------------------------------------------------------------------------ sensitivity
def _composite_changes(mistake):
    n = 0
    for shape in rc.composite_shapes():
        c = rc.get_composite_case(*shape)
        e, m = c.expected(), rc.simulate(c, mistake)
        cmp = ~np.isnan(e["g_sigma"])
        for k in ("weights", "weights_sum", "depth", "image", "g_rgb"):
            n += not np.array_equal(e[k], m[k], equal_nan=True)
        n += not np.array_equal(e["g_sigma"][cmp].astype(F), m["g_sigma"][cmp], equal_nan=True)
    return n


@pytest.mark.parametrize("mistake", rc.MISTAKES)
def test_the_reference_tells_each_classic_mistake_apart(mistake):
    if mistake == "slot_off":
        p = rc.PointsCase(3, 85, 1.0)
        assert not np.array_equal(p.rows(94, 5), p.rows(94, 5, mistake), equal_nan=True)
        assert np.array_equal(p.rows(94, 0), p.rows(94, 0, mistake), equal_nan=True)
    elif mistake == "searchsorted_left":
        c = rc.get_resample_case(5, 4, 7)
        diff = [not np.array_equal(rc.icdf_small(c.z[r], c.sigma[r], c.sd[r], c.u[r]),
                                   rc.icdf_small(c.z[r], c.sigma[r], c.sd[r], c.u[r], left=True)) for r in range(c.N)]
        assert all(diff)
    elif mistake == "ties_new_first":
        c = rc.get_resample_case(5, 4, 7)
        for r in range(c.N):
            new_z = rc.icdf_small(c.z[r], c.sigma[r], c.sd[r], c.u[r])
            for flag in (0, 1):
                a, b = rc.merge_reference(c.z[r], new_z, flag), rc.merge_reference(c.z[r], new_z, flag, new_first=True)
                assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])   # same z_out, another perm
    else:
        assert _composite_changes(mistake) > 0
    if mistake == "pref_carry":                                  # what a lost prefix puts behind the surface: -c_i0 delta
        c = rc.get_composite_case(9, 449, 1, 2, 0)
        r = c.i0.index(0)
        assert c.i1[r] is None
        m, e = rc.simulate(c, mistake)["g_sigma"][r], c.expected()["g_sigma"][r]
        assert np.array_equal(m[:64], e[:64].astype(F)) and not np.array_equal(m[64:], e[64:].astype(F))


def test_the_model_without_a_mistake_is_the_reference():
    assert _composite_changes(None) == 0
