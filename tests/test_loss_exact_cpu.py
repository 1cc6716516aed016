"""The problems of tests/test_loss_exact_gpu.py checked without a GPU (tests/loss_exact_cases.py): the float64 reference is a
second, independent statement of the torch path that golden G13 pins to the reference's own train_step; the conditions that
make tier A exact hold; tier B's bounds are met by the float32 torch path (a bound it could not meet would be wrong)."""
import math

import numpy as np
import pytest
import torch

import loss_exact_cases as lc
from lidarnerf.nerf import loss as loss_mod
from lidarnerf.nerf.loss import LidarLossOptions, lidar_loss, patch_gradient_loss

NAMES = lc.all_names()


def _options(c):
    n = lc.CRIT_NAMES
    return LidarLossOptions(depth_loss=n[c.crit[0]], raydrop_loss=n[c.crit[1]], intensity_loss=n[c.crit[2]],
                            depth_grad_loss=n[c.crit[3]], grad_loss=bool(c.flags & lc.GRAD), sobel_grad=c.sobel,
                            grad_norm_smooth=bool(c.flags & lc.GN), spatial_smooth=bool(c.flags & lc.SPATIAL),
                            tv_loss=bool(c.flags & lc.TV), alpha_grad_norm=c.alphas["a_gn"], alpha_spatial=c.alphas["a_sp"],
                            alpha_tv=c.alphas["a_tv"])


def torch_path(c, dtype, monkeypatch):
    """lidar_loss + patch_gradient_loss of lidarnerf/nerf/loss.py under autograd.  The huber delta of the torch path is tied to
    the scene scale (0.2 * scale); the C struct takes it as a field of its own, so the case's delta is put in its place."""
    real = loss_mod._criterion
    monkeypatch.setattr(loss_mod, "_criterion", lambda name, scale: (
        torch.nn.HuberLoss(reduction="none", delta=c.delta) if name == "huber" else real(name, scale)))
    opts = _options(c)
    gt = torch.as_tensor(c.gt).to(dtype)[None]
    d = torch.as_tensor(c.depth).to(dtype).clone().requires_grad_(True)
    im = torch.as_tensor(c.image).to(dtype).clone().requires_grad_(True)
    a = c.alphas
    loss, pd, gd = lidar_loss({"depth_lidar": d[None], "image_lidar": im[None]}, gt, a["a_d"], a["a_r"], a["a_i"],
                              options=opts, scale=c.scale)
    if c.px > 1:
        loss = loss + patch_gradient_loss(pd, gd, gt[..., 0], c.px, c.py, c.scale, a["a_g"], options=opts)
    loss.backward()
    return float(loss.detach().double()), d.grad.double().numpy(), im.grad.double().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_the_torch_path_in_float64(name, monkeypatch):
    """To 1e-12 of A, the sum of |addends| of each element (= 1e-12 relative wherever an element is a single addend).  The
    case that holds a truth gradient of exactly fl(0.01f) is masked differently by float64 torch (0.0099999998 < 0.01): it is
    compared with the float32 torch path, whose `< 0.01` is the kernels' `< 0.01f`."""
    c, r = lc.get_case(name), lc.ref_of(name)
    if c.f32_threshold:
        loss, gd, gi = torch_path(c, torch.float32, monkeypatch)
        assert abs(loss - r.loss) <= 8 * lc.U * r.A_loss
        assert np.array_equal(gd, r.g_depth) and np.array_equal(gi, r.g_image)
        return
    loss, gd, gi = torch_path(c, torch.float64, monkeypatch)
    assert math.isfinite(loss) and np.isfinite(gd).all() and np.isfinite(gi).all()
    assert abs(loss - r.loss) <= 1e-12 * r.A_loss, (loss, r.loss)
    assert (np.abs(gd - r.g_depth) <= 1e-12 * r.A_gdepth).all(), np.abs(gd - r.g_depth).max()
    assert (np.abs(gi - r.g_image) <= 1e-12 * r.A_gimage).all(), np.abs(gi - r.g_image).max()


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    """Dyadic inputs, powers of two, mask coverage of the Sobel cases; tier A: float32 expectations, sum |terms| within 24 bits of
    one quantum for the loss and for every gradient element."""
    c, r = lc.get_case(name), lc.ref_of(name)
    lc.check_conditions(c, r)
    for what, (idx, val) in c.closed.items():   # the closed forms are the reference's values (one float32 rounding where
        want = getattr(r, what)[idx]            # a count is no power of two)
        assert (np.abs(val - want) <= 2 * lc.U * np.abs(want)).all(), (name, what)
        if lc._pow2(c.N):
            assert np.array_equal(val, want), (name, what)


@pytest.mark.parametrize("name", [n for n in NAMES if lc.get_case(n).tier == "B"])
def test_float32_torch_path_meets_the_bounds_of_tier_b(name, monkeypatch):
    c, r = lc.get_case(name), lc.ref_of(name)
    loss, gd, gi = torch_path(c, torch.float32, monkeypatch)
    ql, qd, qi = lc.ratios(loss, gd, gi, r)
    print(f"{name}: float32 torch error / (2^-24 A): loss {ql:.2f} (K {lc.k_loss(c, 'ex')}), g_depth {qd:.2f} "
          f"(K {lc.k_gdepth(c, 'ex')}), g_image {qi:.2f} (K {lc.k_gimage(c, 'ex')})")
    assert ql <= lc.k_loss(c, "ex") and qd <= lc.k_gdepth(c, "ex") and qi <= lc.k_gimage(c, "ex")


def test_the_case_list_covers_what_it_promises():
    cases = [lc.get_case(n) for n in NAMES]
    shapes = {(c.px, c.py, c.N) for c in cases}
    for px, py, P in lc.SHAPES:
        mine = [c for c in cases if (c.px, c.py, c.N) == (px, py, px * py * P)]
        assert {c.sobel for c in mine} == {False, True}
        assert {c.crit[3] for c in mine if c.flags & lc.GRAD} == {lc.L1, lc.MSE, lc.HUBER, lc.BCE, lc.COS}
        smooth = {c.flags & (lc.GN | lc.SPATIAL | lc.TV) for c in mine}
        assert {lc.GN, lc.SPATIAL, lc.TV, lc.GN | lc.SPATIAL | lc.TV, 0} <= smooth
        assert {k for c in mine for k in c.crit[:3]} == {lc.L1, lc.MSE, lc.HUBER, lc.BCE}
    assert {(3, 5, 525), (17, 16, 544), (2, 8, 1040), (1, 1, 1), (1, 1, 1023), (1, 1, 1024), (1, 1, 1025),
            (1, 1, 256 * 1025)} <= shapes
    c = lc.get_case(lc.STRADDLE + "default")       # patch 17 straddles the first two workgroups, the last one is partly filled
    assert 17 * c.S < lc.WG < 18 * c.S and c.N % lc.WG != 0 and -(-c.N // lc.WG) == 3
    assert lc.get_case("17x16x2_default").S > lc.WG
    assert -(-256 * 1025 // lc.WG) == 1025 > lc.SUM_WG
    tier_a = [c for c in cases if c.tier == "A"]
    assert {c.crit[3] for c in tier_a if c.px > 1} == {lc.L1, lc.MSE, lc.HUBER}
    assert {(c.px, c.py) for c in tier_a} == {(1, 1), (4, 4), (2, 8), (8, 2), (2, 2)}
    for slot in range(3):
        assert {c.crit[slot] for c in tier_a} == {lc.L1, lc.MSE, lc.HUBER}
    assert any(c.entries() == ("ex", "ray") for c in tier_a) and any(c.entries() == ("ex", "patch") for c in tier_a)


def test_the_mask_boundary_floats_are_what_they_claim():
    f, fm = lc.mask_boundary_floats()
    assert np.float32(f) == np.float32(0.01) and f == lc.THRESH and f < 0.01      # float64 torch would take f as in-mask
    assert np.nextafter(np.float32(fm), np.float32(1)) == np.float32(0.01) and fm < f
    c, r = lc.get_case("tie_mask"), lc.ref_of("tie_mask")
    on = np.abs(c.gt[:, 2]) == fm
    assert on.sum() == 4 and (np.abs(c.gt[::2, 2]) >= fm).all() and (c.gt[1::2, 2] == 0).all()
    assert r.mask_on == 4 and r.mask_all == 8


def test_huber_ties_sit_on_both_sides_of_delta():
    c = lc.get_case("tie_huber")
    d = np.abs(c.depth[:11]).astype(np.float32)
    delta = np.float32(c.delta)
    assert (d == delta).sum() == 2 and (d == np.nextafter(delta, np.float32(1))).sum() == 2
    assert (d == np.nextafter(delta, np.float32(0))).sum() == 2
    g = lc.ref_of("tie_huber").g_depth[:11] * c.N / c.alphas["a_d"]
    assert np.array_equal(np.abs(g), np.minimum(np.abs(c.depth[:11]), c.delta))


def test_degenerate_cosine_patches():
    r = lc.ref_of("tie_cos_flat_sobel_1")     # alpha_grad = 1, P = 1, scale 1 / 2: twice float64 torch's 1.4e8 and 1.96e8
    mags = sorted({round(abs(v) / 2 / 1e6) for v in r.g_depth})
    assert mags == [140, 196] and np.isfinite(r.g_depth).all()
    c, r = lc.get_case("tie_cos_dropped_plain"), lc.ref_of("tie_cos_dropped_plain")
    dropped = r.terms[r.tags == "g"][2]
    assert dropped == c.alphas["a_g"] / 4 and (r.g_depth[18:27] == 0).all()
    r = lc.ref_of("tie_cos_flat_plain_4")
    assert (r.A_gdepth == np.abs(r.g_depth)).all()   # nothing but the per-ray addend: the structural gradient is 0


def test_bce_logits():
    c, r = lc.get_case("tie_bce_rays"), lc.ref_of("tie_bce_rays")
    for col in (c.image[:16, 0], c.depth[16:], c.image[16:, 1]):
        assert set(lc.BCE_LOGITS) <= set(col.tolist())
    assert np.isfinite(r.terms).all() and np.isfinite(r.g_depth).all() and np.isfinite(r.g_image).all()
    assert (r.A_gimage[r.A_gimage > 0] >= 2.0 ** -126).all() and (r.A_gdepth[r.A_gdepth > 0] >= 2.0 ** -126).all()


def test_workspace_bytes_at_every_size():
    from lidarnerf import _hip
    L = _hip.lib()
    for N in sorted({lc.get_case(n).N for n in NAMES} | {0, 255, 256, 257, 1 << 26}):
        got = int(L.lnh_lidar_loss_ex_workspace_bytes(N))
        assert got == lc.workspace_bytes(N) and got % 16 == 0 and got >= 4 * -(-N // lc.WG), N
