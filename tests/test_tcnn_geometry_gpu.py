"""Hash grid on tiny-cuda-nn's lattice (kernel gridtype 2) on the GPU: row indices against a Python-integer restatement of
tiny-cuda-nn's published GridEncoding (grid_index / pos_fract; parity with a real tiny-cuda-nn build is unpinned), forward
values against this package's default lattice on a converted table, table / input / TV gradients against float64
restatements, the fused LiDAR chain, load-and-render of a tcnn-layout table, and training."""
import numpy as np
import pytest
import torch

from lidarnerf import tcnn_compat as TC
from lidarnerf.gridencoder import grid

pytestmark = pytest.mark.gpu

SCALE = 0.010784853507573345
H, L, CH = 16, 16, 2
CFG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
       "per_level_scale": TC.per_level_scale(2048, 1)}
PRIMES = [1, 2654435761, 805459861, 3674653429, 2097192037]
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- the restatement (Python integers / float64)
def levels(D, pls, log2):
    """Per level: (scale float32, res, rows, hashed) — tiny-cuda-nn's grid_scale / grid_resolution / offset table."""
    S = np.float32(np.log2(pls))
    cap = 1 << log2
    out = []
    for l in range(L):
        scale = np.float32(np.exp2(np.float64(np.float32(l) * S))) * np.float32(H) - np.float32(1.0)
        res = int(np.ceil(scale)) + 1
        rows = min(-(-res ** D // 8) * 8, cap)
        stride = 1
        for _ in range(D):
            if stride > rows:
                break
            stride *= res
        out.append((np.float32(scale), res, rows, stride > rows))
    return out


def pos_grid(x, scale):
    """pos = fmaf(x, scale, 0.5) in float32 (x * scale is exact in double), its floor and fraction."""
    p = (x.astype(np.float64) * np.float64(scale) + 0.5).astype(np.float32)
    g = np.floor(p)
    return g.astype(np.int64), (p - g).astype(np.float32)


def row_index(g, res, rows, hashed):
    """g [..., D] integer lattice coordinates -> row (tiny-cuda-nn grid_index: hash or dense, then % rows)."""
    D = g.shape[-1]
    if hashed:
        idx = np.zeros(g.shape[:-1], dtype=np.int64)
        for d in range(D):
            idx ^= (g[..., d] * PRIMES[d]) & M32
    else:
        idx = np.zeros(g.shape[:-1], dtype=np.int64)
        s = 1
        for d in range(D):
            idx += g[..., d] * s
            s *= res
        idx &= M32
    return idx % rows


def corners(D):
    return np.array([[(c >> d) & 1 for d in range(D)] for c in range(1 << D)], dtype=np.int64)


def offsets(D, pls, log2):
    return grid.level_offsets(D, L, pls, H, log2, False, gridtype="tcnn")


def _points(D, lv, n_rand, seed):
    r = np.random.default_rng(seed)
    pts = [np.zeros((1, D)), np.ones((1, D)), r.random((n_rand, D))]
    for scale, res, rows, hashed in lv:  # cell boundaries pos = k exactly: x = (k - 0.5) / scale
        k = r.integers(1, res, size=(64, D))
        pts.append(np.clip(((k - 0.5) / float(scale)).astype(np.float32), 0, 1))
        pts.append(np.clip(((k - 0.5) / float(scale)).astype(np.float32) + np.float32(1e-7), 0, 1))
        if not hashed:  # the straddling pair: base corner on row rows - 1 (and the vertices at x = res)
            want = rows - 1
            g = np.array([(want // res ** d) % res for d in range(D)])
            if row_index(g[None], res, rows, False)[0] == want:
                pts.append(np.clip((g[None] + r.random((16, D)) * 0.98 - 0.49) / float(scale), 0, 1))
            pts.append(np.clip(1 - r.random((32, D)) * 1.5 / float(scale), 0, 1))
    return np.ascontiguousarray(np.concatenate(pts).astype(np.float32))


@pytest.mark.parametrize("D", [2, 3, 4])
@pytest.mark.parametrize("desired,log2", [(2048, 19), (32768, 19)])
def test_corner_indices_match_tiny_cuda_nn_restatement(desired, log2, D):
    from gpu_util import call, dev, host
    pls = TC.per_level_scale(desired, 1)
    lv = levels(D, pls, log2)
    off = offsets(D, pls, log2)
    assert np.diff(off).tolist() == [rows for _, _, rows, _ in lv]
    x = _points(D, lv, 4000, D * 7 + log2)
    out = torch.empty((L, x.shape[0], 1 << D), dtype=torch.int32, device="cuda")
    call("lnh_grid_corner_indices", dev(x), torch.from_numpy(off), out, x.shape[0], D, CH, L,
         float(np.log2(pls)), H, 2, 0)
    got = host(out).view(np.uint32).astype(np.int64)
    cs = corners(D)
    n_straddle = 0
    for l, (scale, res, rows, hashed) in enumerate(lv):
        g, _ = pos_grid(x, scale)
        want = row_index(g[:, None, :] + cs[None], res, rows, hashed) * CH
        np.testing.assert_array_equal(got[l], want, err_msg=f"level {l}")
        if not hashed:
            n_straddle += int((row_index(g, res, rows, False) == rows - 1).sum())
    assert n_straddle > 0  # the wrap was exercised


def test_align_corners_and_unknown_gridtype_refused():
    from lidarnerf import _hip
    from gpu_util import dev
    pls = CFG["per_level_scale"]
    off = torch.from_numpy(offsets(3, pls, 19))
    x = dev(np.full((4, 3), 0.5, np.float32))
    out = torch.empty((L, 4, 8), dtype=torch.int32, device="cuda")
    for gt, al in ((2, 1), (3, 0)):
        rc = _hip.lib().lnh_grid_corner_indices(x.data_ptr(), off.data_ptr(), out.data_ptr(), 4, 3, CH, L,
                                                float(np.log2(pls)), H, gt, al, _hip.stream())
        assert rc != 0
    assert _hip.lib().lnh_version() >= 101


def _fwd(x, table, off, S, gridtype, interp, dydx):
    from gpu_util import call
    B, D = x.shape
    out = torch.empty((L, B, CH), dtype=table.dtype, device="cuda")
    dy = torch.empty((B, L * D * CH), dtype=table.dtype, device="cuda") if dydx else None
    call("lnh_grid_encode_forward", x, table, off, out, B, D, CH, L, S, H, dy, gridtype, 0, interp,
         0 if table.dtype == torch.float32 else 1)
    torch.cuda.synchronize()
    return out, dy


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("interp", [0, 1])
def test_forward_equals_default_lattice_on_converted_table(dtype, interp):
    """lnh_grid_encode_forward(gridtype 2, T) == lnh_grid_encode_forward(gridtype 0, convert_tcnn_hashgrid_params(T)): the
    same corner values with the same weights in the same order, bit for bit (linear: the plain kernel classes; smoothstep and
    dy_dx: the generic ones)."""
    from gpu_util import dev
    pls = CFG["per_level_scale"]
    S = float(np.log2(pls))
    lv = levels(3, pls, 19)
    off_t = torch.from_numpy(offsets(3, pls, 19))
    off_m = torch.from_numpy(grid.level_offsets(3, L, pls, H, 19, False))
    n = TC._tcnn_hashgrid_param_count(CFG, 3)
    T = (torch.rand(n, generator=torch.Generator().manual_seed(5)) - 0.5)
    Tm = TC.convert_tcnn_hashgrid_params(T, CFG, 3)
    x = dev(_points(3, lv, 200_000, 11))
    tt, tm = T.view(-1, CH).to(dtype).cuda(), Tm.view(-1, CH).to(dtype).cuda()
    for dydx in (False, True):
        a, da = _fwd(x, tt, off_t, S, 2, interp, dydx)
        b, db = _fwd(x, tm, off_m, S, 0, interp, dydx)
        assert torch.equal(a, b)
        if dydx:
            assert torch.equal(da, db)


def _scatter64(x, g, lv, offs, rows_total):
    """float64 table gradient: every corner's w * g added onto its tiny-cuda-nn row (aliased rows included)."""
    out = np.zeros((rows_total, CH))
    cs = corners(3)
    for l, (scale, res, rows, hashed) in enumerate(lv):
        gi, fr = pos_grid(x, scale)
        fr = fr.astype(np.float64)
        for c in cs:
            w = np.prod(np.where(c[None] == 1, fr, 1 - fr), axis=1)
            r = row_index(gi + c[None], res, rows, hashed) + offs[l]
            np.add.at(out, r, w[:, None] * g[l])
    return out


def test_table_gradient_atomic_and_bucketed_against_float64():
    from gpu_util import call, dev, host
    pls = CFG["per_level_scale"]
    S = float(np.log2(pls))
    lv = levels(3, pls, 19)
    offs = offsets(3, pls, 19)
    off = torch.from_numpy(offs)
    rows_total = int(offs[-1])
    r = np.random.default_rng(3)
    # random points (straddling pairs included) and consecutive samples along rays: the latter merge into runs on the
    # dense levels, whose rows the paired scatter deals to 128-row groups
    o = r.random((300, 1, 3)) * 0.4 + 0.3
    dr = r.standard_normal((300, 1, 3))
    dr /= np.linalg.norm(dr, axis=-1, keepdims=True)
    rays = np.clip(o + dr * np.linspace(0.0, 0.3, 128)[None, :, None], 0, 1).reshape(-1, 3)
    x = np.ascontiguousarray(np.concatenate([_points(3, lv, 60_000, 13), rays.astype(np.float32)]))
    B = x.shape[0]
    g = (r.standard_normal((L, B, CH)) * 0.1).astype(np.float32)
    want = _scatter64(x, g.astype(np.float64), lv, offs, rows_total)
    xd, gd = dev(x), dev(g)
    ge = torch.zeros((rows_total, CH), device="cuda")
    call("lnh_grid_encode_backward", gd, xd, None, off, ge, B, 3, CH, L, S, H, None, None, 2, 0, 0, 0)
    tol = 1e-5 * np.abs(want).max()
    np.testing.assert_allclose(host(ge), want, rtol=1e-4, atol=tol)
    outs = []
    for _ in range(2):
        gb, _ = grid.grid_backward_raw(gd, xd, rows_total, off, S, H, 2, False, 0, None)
        outs.append(gb)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    np.testing.assert_allclose(host(outs[0]), want, rtol=1e-4, atol=tol)
    # the straddling rows got their gradient: row 0 of every dense level holds aliased contributions
    dense = [l for l, v in enumerate(lv) if not v[3]]
    assert dense and all(np.abs(want[offs[l]]).sum() > 0 for l in dense)


def test_input_gradient_and_tv_against_float64():
    from gpu_util import call, dev, host
    pls = CFG["per_level_scale"]
    S = float(np.log2(pls))
    lv = levels(3, pls, 19)
    offs = offsets(3, pls, 19)
    off = torch.from_numpy(offs)
    rows_total = int(offs[-1])
    r = np.random.default_rng(8)
    table = (r.random((rows_total, CH)) - 0.5).astype(np.float32)
    x = _points(3, lv, 3000, 17)
    B = x.shape[0]
    # d out / d x (linear): scale * sum over the 4 edges along dimension gd of (T[c | gd] - T[c]) * weight of the others
    _, dy = _fwd(dev(x), dev(table), off, S, 2, 0, True)
    got = host(dy).reshape(B, L, 3, CH)
    cs = corners(3)
    want = np.zeros((B, L, 3, CH))
    for l, (scale, res, rows, hashed) in enumerate(lv):
        gi, fr = pos_grid(x, scale)
        fr = fr.astype(np.float64)
        for gd in range(3):
            for c in cs[cs[:, gd] == 0]:
                w = np.prod([np.where(c[d] == 1, fr[:, d], 1 - fr[:, d]) for d in range(3) if d != gd], axis=0)
                c1 = c.copy()
                c1[gd] = 1
                t0 = table[row_index(gi + c[None], res, rows, hashed) + offs[l]].astype(np.float64)
                t1 = table[row_index(gi + c1[None], res, rows, hashed) + offs[l]].astype(np.float64)
                want[:, l, gd] += float(scale) * w[:, None] * (t1 - t0)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())
    # total-variation gradient (gridencoder.cu:695-807's rule on this lattice: +-1 neighbours along each dimension)
    xt = x[:400]
    tg = torch.zeros((rows_total, CH), device="cuda")
    weight = 1e-2
    call("lnh_grad_total_variation", dev(xt), dev(table), tg, off, weight, xt.shape[0], 3, CH, L, S, H, 2, 0, 0)
    wt = np.zeros((rows_total, CH))
    for l, (scale, res, rows, hashed) in enumerate(lv):
        gi, _ = pos_grid(xt, scale)
        for b in range(xt.shape[0]):
            p = gi[b].copy()
            i0 = row_index(p[None], res, rows, hashed)[0] + offs[l]
            acc, idel = np.zeros(CH), np.zeros(CH)
            for d in range(3):
                for step, okd in ((1, p[d] < res), (-1, p[d] > 0)):
                    if okd:
                        q = p.copy()
                        q[d] += step
                        diff = table[i0].astype(np.float64) - table[row_index(q[None], res, rows, hashed)[0] + offs[l]]
                        acc += diff
                        idel += diff * diff
            wt[i0] += weight / 6 * acc / np.sqrt(idel + 1e-9)
    np.testing.assert_allclose(host(tg), wt, rtol=1e-3, atol=1e-4 * np.abs(wt).max())


def _rays(N, seed):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(N, 3, generator=g) - 0.5) * 0.1
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    return o, d


def _tcnn_net(geometry, seed=3, table_scale=0.3, desired=32768):
    from lidarnerf.nerf.network_tcnn import NeRFNetwork
    torch.manual_seed(seed)
    net = NeRFNetwork(encoding="hashgrid", desired_resolution=desired, bound=1, min_near=SCALE, min_near_lidar=SCALE,
                      tcnn_geometry=geometry)
    with torch.no_grad():
        net.encoder.impl.params.uniform_(-table_scale, table_scale)
    return net.cuda().eval()


def test_fused_chain_matches_modular_path_in_tcnn_geometry():
    """test_tcnn_facade_fused_step_matches_modular_path's comparison on a tcnn-geometry field.  (The ragged / occupancy
    chain is not reached: network_tcnn renders without cuda_ray here, as the reference's -L run does.)"""
    from lidarnerf.nerf import fused
    from lidarnerf.nerf.train_step import lidar_loss
    net = _tcnn_net("tcnn", seed=5)
    assert net.encoder.impl.gridtype_id == 2 and not net.cuda_ray
    assert not fused.ragged_supported(net)  # the occupancy chain is gated to gridtype 0
    o, d = _rays(48, 19)
    gt = torch.rand(1, 48, 3, generator=torch.Generator().manual_seed(21)).cuda()
    gt[..., 0] = (gt[..., 0] > 0.2).float()
    assert fused.supported(net, True, 768, 64)

    def run(fused_flag):
        net.fused_lidar = fused_flag
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.render(o.cuda()[None], d.cuda()[None], cal_lidar_color=True, staged=False, perturb=False,
                             num_steps=768, upsample_steps=64)
            loss, _, _ = lidar_loss(out, gt)
        (loss * 64.0).backward()
        grads = {n: p.grad.detach().float().clone() for n, p in net.named_parameters() if p.grad is not None}
        return {k: v.detach().float() for k, v in out.items()}, loss.detach().float(), grads

    out_f, loss_f, g_f = run(True)
    out_m, loss_m, g_m = run(False)
    for k in ("depth_lidar", "image_lidar", "weights_sum_lidar"):
        torch.testing.assert_close(out_f[k], out_m[k], rtol=2e-3, atol=2e-4, msg=k)
    torch.testing.assert_close(loss_f, loss_m, rtol=2e-3, atol=1e-4)
    assert set(g_f) == set(g_m) == {"encoder.impl.params", "sigma_net.params", "lidar_color_net.params"}
    for k in g_m:
        rel = (g_f[k] - g_m[k]).norm() / (g_m[k].norm() + 1e-12)
        assert rel < 3e-2, (k, rel.item())


def test_tcnn_layout_table_loads_natively_and_renders_like_its_conversion(monkeypatch):
    """A table in tiny-cuda-nn layout: loaded natively into a tcnn-geometry model, and converted into a default-geometry
    model (LNH_TCNN_CONVERT=1).  Encoder outputs bit-identical, rendered depth within 1e-6 relative."""
    monkeypatch.setenv("LNH_TCNN_CONVERT", "1")
    a = _tcnn_net("tcnn", seed=7, desired=2048)
    b = _tcnn_net("torch-ngp", seed=7, desired=2048)
    cfg = a.encoder.encoding_config
    n = TC._tcnn_hashgrid_param_count(cfg, 3)
    sd = a.state_dict()
    assert sd["encoder.params"].numel() == n
    sd["encoder.params"] = (torch.rand(n, generator=torch.Generator().manual_seed(9)) - 0.5) * 0.6
    a.load_state_dict(sd)
    with pytest.warns(UserWarning, match="converting"):
        b.load_state_dict(sd)
    x = torch.rand(300_000, 3, device="cuda")
    with torch.no_grad():
        assert torch.equal(a.encoder(x), b.encoder(x))
        o, d = _rays(64, 23)
        ra = a.render(o.cuda()[None], d.cuda()[None], cal_lidar_color=True, staged=False, perturb=False, num_steps=128,
                      upsample_steps=32)
        rb = b.render(o.cuda()[None], d.cuda()[None], cal_lidar_color=True, staged=False, perturb=False, num_steps=128,
                      upsample_steps=32)
    torch.testing.assert_close(ra["depth_lidar"], rb["depth_lidar"], rtol=1e-6, atol=0)


def _train(steps, graph, ckpt=None, resume=None):
    import bench
    from lidarnerf.nerf.network_tcnn import NeRFNetwork
    from lidarnerf.nerf.train_step import LidarTrainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = NeRFNetwork(encoding="hashgrid", desired_resolution=32768, log2_hashmap_size=19, bound=1, min_near=SCALE,
                        min_near_lidar=SCALE, bg_radius=-1, tcnn_geometry="tcnn").to(dev).train()
    tr = LidarTrainer(model, lr=1e-2, iters=30000, fp16=True, scale=bench.SCALE, graph=graph,
                      render_kwargs=dict(num_steps=768, upsample_steps=64))
    assert tr.table is not None  # the fused table optimizer
    poses = bench.synthetic_frames(8, dev)
    batches = [bench.make_batch(poses, s, 1024, 0, dev, (1, 1), "analytic") for s in range(8)]
    if resume is not None:
        tr.load_checkpoint(resume)
    torch.manual_seed(11)
    losses = [tr.step(*batches[s % 8]).detach().clone() for s in range(steps)]
    if ckpt is not None:
        tr.save_checkpoint(ckpt)
    torch.cuda.synchronize()
    state = [tr.table.detach().clone(), tr.t_m.clone(), tr.t_v.clone()] + [p.detach().clone() for p in tr.small]
    return state, (torch.stack(losses) if losses else None), tr, batches


def test_training_is_reproducible_learns_and_resumes(tmp_path):
    a, la, _, _ = _train(100, graph=False, ckpt=str(tmp_path / "a.pth"))
    c, lc, _, _ = _train(100, graph=True)
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    assert torch.equal(la, lc)
    la = la.float().cpu().numpy()
    assert np.isfinite(la).all() and la[-20:].mean() < la[:20].mean()
    ck = torch.load(str(tmp_path / "a.pth"), weights_only=False)
    assert ck["model"]["encoder.params"].numel() == TC._tcnn_hashgrid_param_count(
        {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
         "per_level_scale": TC.per_level_scale(32768, 1)}, 3)
    # save -> fresh trainer -> load: the next step equals the next step of the run that saved
    _, _, tr1, b1 = _train(100, graph=False)
    torch.manual_seed(99)
    nxt = tr1.step(*b1[100 % 8]).detach().clone()
    _, _, tr2, b2 = _train(0, graph=False, resume=str(tmp_path / "a.pth"))
    torch.manual_seed(99)
    got = tr2.step(*b2[100 % 8]).detach().clone()
    torch.cuda.synchronize()
    assert torch.equal(nxt, got)
    assert torch.equal(tr1.table, tr2.table)
