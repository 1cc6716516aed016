"""Per-ray LiDAR compositing / resampling kernels vs the torch restatement of renderer.py (oracle/render_ref.py),
which itself is pinned against the imported reference by tests/golden (G1, G2)."""
import os

import numpy as np
import pytest
import torch

from oracle import render_ref

pytestmark = pytest.mark.gpu
SCALE = 0.010784853507573345


def _ray_inputs(N, T, seed, K=2):
    g = torch.Generator().manual_seed(seed)
    near, far = SCALE, 81 * SCALE
    z = torch.linspace(0, 1, T).expand(N, T) * (far - near) + near
    sd = torch.full((N,), (far - near) / T)
    z = z + (torch.rand(N, T, generator=g) - 0.5) * sd[:, None]
    centre = torch.rand(N, 1, generator=g) * 0.6 + 0.1
    sigma = 3.0 + 400.0 * torch.exp(-((z - centre) / 0.01) ** 2) * (torch.rand(N, 1, generator=g) > 0.2)
    sigma[0] = 0.0           # empty ray
    sigma[1] = 1e6           # fully opaque at the first sample
    rgb = torch.rand(N, T, K, generator=g)
    return z.contiguous(), sigma.contiguous(), rgb.contiguous(), sd


@pytest.mark.parametrize("N,T", [(37, 832), (5, 64), (3, 100), (2, 2)])
def test_weights_and_composite_forward(N, T):
    from gpu_util import call
    z, sigma, rgb, sd = _ray_inputs(N, T, 1)
    w_ref, _ = render_ref.weights_from_sigma(z, sigma, sd[:, None])
    zc, sc, cc, sdc = z.cuda(), sigma.cuda(), rgb.cuda(), sd.cuda()
    w = torch.empty((N, T), device="cuda")
    call("lnh_lidar_weights", zc, sc, sdc, N, T, 1.0, w)
    torch.testing.assert_close(w.cpu(), w_ref, rtol=2e-5, atol=1e-7)
    ws = torch.empty(N, device="cuda")
    dep = torch.empty(N, device="cuda")
    img = torch.empty((N, 2), device="cuda")
    w2 = torch.empty((N, T), device="cuda")
    call("lnh_lidar_composite_forward", zc, sc, cc, sdc, N, T, 2, 1.0, w2, ws, dep, img)
    torch.testing.assert_close(w2.cpu(), w_ref, rtol=2e-5, atol=1e-7)
    torch.testing.assert_close(ws.cpu(), w_ref.sum(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dep.cpu(), (w_ref * z).sum(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(img.cpu(), (w_ref[..., None] * rgb).sum(-2), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("T", [1, 2, 65, 449, 897])
def test_every_dense_walker_returns_the_same_weights(T):
    """lnh_lidar_weights, lnh_lidar_composite_forward, lnh_lidar_merge_weights (identity perm) and
    lnh_lidar_color_composite_forward walk a ray with the one definition of csrc/transmittance.h: the same weights bit for
    bit on general alphas (the exact known-answer tests use alpha in {0, 1}, which cannot tell alpha * (carry * excl) from
    (alpha * carry) * excl), and equal weights_sum / depth from the two compositing entry points.  N = 5: the second
    workgroup holds a lone ray; T = 449 / 897: one sample past one / two groups of seven 64-sample rounds."""
    from gpu_util import call
    N, ds = 5, 2.0
    g = torch.Generator().manual_seed(100 + T)
    z = torch.sort(torch.rand(N, T, generator=g) * 0.8 + 0.01, dim=1)[0]
    sigma = torch.rand(N, T, generator=g) * 4
    sd = 0.8 / T * (1 + torch.arange(N, dtype=torch.float32) / 8)
    # the data is not degenerate: the float64 restatement of the weights has general alphas and visible weights everywhere
    z64, s64 = z.double().numpy(), sigma.double().numpy()
    delta = np.concatenate([np.diff(z64, axis=1), sd.double().numpy()[:, None]], axis=1)
    alpha = 1.0 - np.exp(-delta * ds * s64)
    trans = np.cumprod(np.concatenate([np.ones((N, 1)), 1.0 - alpha + 1e-15], axis=1), axis=1)
    w64 = alpha * trans[:, :-1]
    assert (w64 > 1e-8).mean() >= 0.95
    if T >= 2:
        assert ((alpha > 1e-6) & (alpha < 0.999)).mean() >= 0.95
    if T >= 65:
        assert trans[:, -1].min() > 0.03

    zc, sc, sdc = z.cuda(), sigma.cuda(), sd.cuda()
    perm = torch.arange(T, dtype=torch.int32).expand(N, T).contiguous().cuda()
    h16 = (torch.randn(N * T, 16, generator=g) * 0.5).half().cuda()
    cdir = torch.randn(N, 64, generator=g).cuda()
    w16 = (torch.randn(64 * 16 + 64 * 64 + 16 * 64, generator=g) * 0.2).half().cuda()
    rgb = torch.rand(N, T, 2, generator=g).cuda()

    def new(*shape):
        return torch.full(shape, float("nan"), device="cuda")
    w_a, w_b, w_c, w_d = new(N, T), new(N, T), new(N, T), new(N, T)
    ws_b, dp_b, im_b, ws_d, dp_d, im_d = new(N), new(N), new(N, 2), new(N), new(N), new(N, 2)
    sig_c, sig_d, rgb_d = new(N, T), new(N, T), new(N, T, 2)
    call("lnh_lidar_weights", zc, sc, sdc, N, T, ds, w_a)
    call("lnh_lidar_composite_forward", zc, sc, rgb, sdc, N, T, 2, ds, w_b, ws_b, dp_b, im_b)
    call("lnh_lidar_merge_weights", zc, sc, perm, sdc, N, T, ds, sig_c, w_c)
    call("lnh_lidar_color_composite_forward", zc, sc, perm, sdc, h16, cdir, w16, N, T, ds, sig_d, w_d, rgb_d, ws_d, dp_d, im_d)
    # they are the weights, not merely equal.  float32 against float64: alpha = 1 - e is two roundings near 1 (2 * 2^-24
    # absolute), T_i a product of up to 897 rounded factors (897 * 2^-24 = 5.4e-5 relative)
    np.testing.assert_allclose(w_a.cpu().numpy(), w64, rtol=1e-4, atol=2e-7)
    assert torch.equal(w_b, w_a) and torch.equal(w_c, w_a) and torch.equal(w_d, w_a)
    assert torch.equal(sig_c, sc) and torch.equal(sig_d, sc)
    assert torch.equal(ws_d, ws_b) and torch.equal(dp_d, dp_b)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_composite_backward_matches_autograd(K):
    from gpu_util import call
    N, T = 29, 832
    z, sigma, rgb, sd = _ray_inputs(N, T, 2, K)
    sigma = sigma.clamp(max=2000.0)  # keep 1-alpha away from exact 0 (there the reference gradient is 0/0-ish too)
    sg = sigma.double().requires_grad_(True)
    cg = rgb.double().requires_grad_(True)
    w, _ = render_ref.weights_from_sigma(z.double(), sg, sd.double()[:, None])
    ws, dep, img = w.sum(-1), (w * z.double()).sum(-1), (w[..., None] * cg).sum(-2)
    g = torch.Generator().manual_seed(5)
    gws, gdp, gim = torch.randn(N, generator=g), torch.randn(N, generator=g) * 50, torch.randn(N, K, generator=g)
    (ws * gws.double()).sum().add((dep * gdp.double()).sum()).add((img * gim.double()).sum()).backward()
    gs = torch.empty((N, T), device="cuda")
    gc = torch.empty((N, T, K), device="cuda")
    call("lnh_lidar_composite_backward", gws.cuda(), gdp.cuda(), gim.cuda(), z.cuda(), sigma.cuda(), rgb.cuda(),
         sd.cuda(), N, T, K, 1.0, gs, gc)
    scale = sg.grad.abs().max().item()
    torch.testing.assert_close(gs.cpu().double(), sg.grad, rtol=2e-3, atol=2e-5 * scale)
    torch.testing.assert_close(gc.cpu().double(), cg.grad, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("N,T,n_new", [(41, 768, 64), (7, 128, 128), (3, 50, 7)])
def test_resample_merge(det, N, T, n_new):
    from gpu_util import call
    z, sigma, _, sd = _ray_inputs(N, T, 3)
    if det:
        u = torch.linspace(0.5 / n_new, 1 - 0.5 / n_new, n_new).expand(N, n_new).contiguous()
    else:
        u = torch.rand(N, n_new, generator=torch.Generator().manual_seed(4))
    w, deltas = render_ref.weights_from_sigma(z, sigma, sd[:, None])
    z_mid = z[..., :-1] + 0.5 * deltas[..., :-1]
    new_ref = render_ref.sample_pdf(z_mid, w[:, 1:-1], n_new, det=det, u=u)
    new_z = torch.empty((N, n_new), device="cuda")
    z_out = torch.empty((N, T + n_new), device="cuda")
    perm = torch.empty((N, T + n_new), dtype=torch.int32, device="cuda")
    call("lnh_lidar_resample", z.cuda(), sigma.cuda(), sd.cuda(), u.cuda(), N, T, n_new, 1.0, 0, new_z, z_out, perm)
    # cdf is a float32 running sum evaluated in a different association order than torch.cumsum: positions agree to
    # a few ulp of the bin width
    # (an ulp of cdf is amplified by 1/denom inside steep bins, hence the absolute bound of ~4% of a bin width;
    #  the bulk agrees far tighter)
    err = (new_z.cpu() - new_ref).abs()
    assert err.max().item() < 4e-5, err.max().item()
    assert torch.quantile(err.flatten(), 0.99).item() < 3e-6
    # the merge must be EXACTLY a sort of the concatenation the kernel itself produced
    cat = torch.cat([z.cuda(), new_z], dim=1)
    zs, _ = torch.sort(cat, dim=1)
    assert torch.equal(z_out, zs)
    assert torch.equal(torch.gather(cat, 1, perm.long()), z_out)
    assert torch.equal(torch.sort(perm, dim=1)[0], torch.arange(T + n_new, device="cuda", dtype=torch.int32).expand(N, -1))


def test_resample_sorted_new_samples():
    """sorted_new = 1: same sample SET, emitted ascending, permutation consistent with the new slot order."""
    from gpu_util import call
    N, T, n_new = 33, 768, 64
    z, sigma, _, sd = _ray_inputs(N, T, 5)
    u = torch.rand(N, n_new, generator=torch.Generator().manual_seed(6))
    outs = []
    for flag in (0, 1):
        new_z = torch.empty((N, n_new), device="cuda")
        z_out = torch.empty((N, T + n_new), device="cuda")
        perm = torch.empty((N, T + n_new), dtype=torch.int32, device="cuda")
        call("lnh_lidar_resample", z.cuda(), sigma.cuda(), sd.cuda(), u.cuda(), N, T, n_new, 1.0, flag, new_z, z_out, perm)
        outs.append((new_z, z_out, perm))
    (nz0, zo0, p0), (nz1, zo1, p1) = outs
    assert torch.equal(torch.sort(nz0, dim=1)[0], nz1)
    assert torch.equal(zo0, zo1)
    cat = torch.cat([z.cuda(), nz1], dim=1)
    assert torch.equal(torch.gather(cat, 1, p1.long()), zo1)


def test_resample_strided_reads_the_first_columns_of_a_wider_buffer():
    """lnh_lidar_resample_strided on the [N, T+n] buffer the fused step keeps == lnh_lidar_resample on a contiguous copy of
    its first T columns, bit for bit; a stride below T is refused."""
    from gpu_util import call
    from lidarnerf import _hip
    N, T, n_new = 19, 768, 64
    z, sigma, _, sd = _ray_inputs(N, T, 11)
    u = torch.rand(N, n_new, generator=torch.Generator().manual_seed(12))
    wide = torch.full((N, T + n_new), float("nan"))
    wide[:, :T] = sigma
    outs = []
    for strided in (False, True):
        new_z = torch.empty((N, n_new), device="cuda")
        z_out = torch.empty((N, T + n_new), device="cuda")
        perm = torch.empty((N, T + n_new), dtype=torch.int32, device="cuda")
        if strided:
            call("lnh_lidar_resample_strided", z.cuda(), wide.cuda(), T + n_new, sd.cuda(), u.cuda(), N, T, n_new, 1.0, 1,
                 new_z, z_out, perm)
        else:
            call("lnh_lidar_resample", z.cuda(), sigma.cuda(), sd.cuda(), u.cuda(), N, T, n_new, 1.0, 1, new_z, z_out, perm)
        outs.append((new_z, z_out, perm))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="sigma_stride"):
        call("lnh_lidar_resample_strided", z.cuda(), wide.cuda(), T - 1, sd.cuda(), u.cuda(), N, T, n_new, 1.0, 1,
             outs[0][0], outs[0][1], outs[0][2])


def test_resample_points_writes_the_coordinates_of_the_new_samples():
    """lnh_lidar_resample_points == lnh_lidar_resample_strided(sorted_new = 1) + lnh_lidar_sample_points of the new depths,
    bit for bit; the coarse rows of the coordinate buffer are left alone."""
    from gpu_util import call
    N, T, n_new = 23, 768, 64
    z, sigma, _, sd = _ray_inputs(N, T, 13)
    g = torch.Generator().manual_seed(14)
    u = torch.rand(N, n_new, generator=g).cuda()
    o = ((torch.rand(N, 3, generator=g) - 0.5) * 0.05).cuda()
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).cuda()
    aabb = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32).cuda()
    wide = torch.zeros(N, T + n_new)
    wide[:, :T] = sigma
    outs = []
    for fused in (False, True):
        new_z = torch.empty((N, n_new), device="cuda")
        z_out = torch.empty((N, T + n_new), device="cuda")
        perm = torch.empty((N, T + n_new), dtype=torch.int32, device="cuda")
        x01 = torch.full((N * (T + n_new), 3), float("nan"), device="cuda")
        if fused:
            call("lnh_lidar_resample_points", z.cuda(), wide.cuda(), T + n_new, sd.cuda(), u, N, T, n_new, 1.0, new_z, z_out,
                 perm, o, d, aabb, 1.0, x01)
        else:
            call("lnh_lidar_resample_strided", z.cuda(), wide.cuda(), T + n_new, sd.cuda(), u, N, T, n_new, 1.0, 1, new_z,
                 z_out, perm)
            call("lnh_lidar_sample_points", o, d, new_z, aabb, 1.0, N, n_new, T + n_new, T, x01)
        outs.append((new_z, z_out, perm, torch.nan_to_num(x01, nan=-7.0)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool((outs[1][3].view(N, T + n_new, 3)[:, :T] == -7.0).all())


def test_resample_against_reference_golden(golden_dir):
    """G1: reference sample_pdf outputs.  First the properties on a random smooth ray (monotone in u, inside the ray); then the
    golden rows themselves, reproduced through sigma, against the reference's `rnd` and `det`."""
    from gpu_util import call
    g = np.load(os.path.join(golden_dir, "g1_sample_pdf.npz"))
    bins = torch.from_numpy(g["bins"])  # [B, 767] z_mid; rebuild z so that z_mid(z) == bins is not needed: only
    # property checked: outputs lie inside [bins.min, bins.max] of the kernel's own z_mid and are monotone in u (det)
    N, T = 8, 768
    z, sigma, _, sd = _ray_inputs(N, T, 9)
    u = torch.linspace(0.5 / 64, 1 - 0.5 / 64, 64).expand(N, 64).contiguous()
    new_z = torch.empty((N, 64), device="cuda")
    z_out = torch.empty((N, T + 64), device="cuda")
    perm = torch.empty((N, T + 64), dtype=torch.int32, device="cuda")
    call("lnh_lidar_resample", z.cuda(), sigma.cuda(), sd.cuda(), u.cuda(), N, T, 64, 1.0, 0, new_z, z_out, perm)
    nz = new_z.cpu()
    assert torch.all(nz[:, 1:] >= nz[:, :-1])
    assert torch.all(nz >= z[:, :1]) and torch.all(nz <= z[:, -1:])
    assert bins.shape[1] == 767
    # The comparison with the reference's own outputs: the golden weights fed through the sigma that reproduces them and a z
    # whose midpoints are the golden bins (render_exact_cases.g1_inputs: the rows whose weights can be compositing weights),
    # with G1's u against `rnd` and with the deterministic u against `det`, within the derived bound of the inverse cdf
    # (render_exact_cases.icdf_reference, float64 on the kernel's inputs) plus the reference's own float32 deviation from
    # float64 on the golden data and the float64 distance between the two sets of inputs.
    import render_exact_cases as rc
    zk, sk, sdk, rows = rc.g1_inputs(g["bins"], g["weights"])
    assert list(rows) == [3, 5] and g["weights"][3].max() == 0.0 and g["weights"][5].sum() == 1.0
    zm = zk.astype(np.float64)[:, :-1] + 0.5 * np.diff(zk.astype(np.float64), axis=1)
    assert np.abs(zm - g["bins"][rows]).max() < 2.0 ** -23                 # midpoints of the float32 z = the golden bins
    B = len(rows)
    for name, uk in (("rnd", g["u"][rows]), ("det", u[:B].numpy())):
        ref = rc.icdf_reference(zk, sk, sdk, 1.0, uk)
        gold = g[name][rows].astype(np.float64)
        gold64 = render_ref.sample_pdf(torch.from_numpy(g["bins"][rows]).double(), torch.from_numpy(g["weights"][rows]).double(),
                                       64, u=torch.from_numpy(uk).double()).numpy()
        own, moved = np.abs(gold - gold64), np.abs(gold64 - ref["s"])
        assert own.max() < 1e-6 and moved.max() < 1e-7 and not ref["excluded"].any()
        nz, zo, pm = (torch.empty((B, 64), device="cuda"), torch.empty((B, T + 64), device="cuda"),
                      torch.empty((B, T + 64), dtype=torch.int32, device="cuda"))
        call("lnh_lidar_resample", torch.from_numpy(zk).cuda(), torch.from_numpy(sk).cuda(), torch.from_numpy(sdk).cuda(),
             torch.from_numpy(np.ascontiguousarray(uk)).cuda(), B, T, 64, 1.0, 0, nz, zo, pm)
        err = np.abs(nz.cpu().numpy().astype(np.float64) - gold)
        share = float((err / (ref["bound"] + own + moved)).max())
        print(f"[bound] G1 {name}: max |new_z - golden| = {err.max():.3e}, {share:.3f} of the bound")
        assert share <= 1.0, (name, share)
