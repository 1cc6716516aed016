"""Alive-ray evaluation of LiDAR rays (csrc/lidar_infer.hip, NeRFRenderer.run_cuda_alive): the round's three entry points
against the C oracle's training marcher (bit for bit) and a float64 restatement of the compositor written here, and the
renderer's new evaluation path against the existing one (run_cuda in eval mode)."""
import math

import numpy as np
import pytest
import torch

from oracle import c_oracle

pytestmark = pytest.mark.gpu
SCALE = 0.005
T_THRESH = 1e-4


def _say(*a):
    print("[lidar_infer]", *a, flush=True)


# ------------------------------------------------------------------------------------------------ scenes (test_raymarch_gpu)
def _scene(cascade):
    Hh = 128
    r = np.random.default_rng(3)
    dens = np.zeros(cascade * Hh ** 3, np.float32)
    idx = np.arange(Hh ** 3, dtype=np.int32)
    xyz = (c_oracle.morton3D_invert(idx).astype(np.float32) + 0.5) / Hh * 2 - 1
    for cas in range(cascade):
        rr = np.linalg.norm(xyz * (2 ** cas), axis=1)
        dens[cas * Hh ** 3:(cas + 1) * Hh ** 3][(rr < 0.6 * 2 ** cas) & (r.random(Hh ** 3) < 0.7)] = 1.0
    return c_oracle.packbits(dens, 0.01), Hh


def _rays(N, bound, seed):
    r = np.random.default_rng(seed)
    o = (r.standard_normal((N, 3)) * 0.05 + np.array([-0.8 * bound, 0.1, 0.0])).astype(np.float32)
    d = r.standard_normal((N, 3)).astype(np.float32)
    d[:, 0] = np.abs(d[:, 0]) + 0.7
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[::13] += np.array([0.0, 5.0 * bound, 0.0], np.float32)   # these miss the box
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    wn, wf = c_oracle.near_far_from_aabb(o, d, aabb, 0.05)
    wf[5::13] = wn[5::13] * 0.5                                # far in front of near: no lattice point is visited
    return o, d, wn, wf


class _Loop:
    """The caller's side of the alive loop over the raw entry points, with host mirrors of every buffer per round."""

    def __init__(self, o, d, near, far, bits, bound, cascade, Hh, dt_gamma, K=2, max_steps=1024):
        from gpu_util import dev
        self.N = N = o.shape[0]
        self.o, self.d, self.bits, self.far = dev(o), dev(d), dev(bits), dev(far)
        self.geo = (bound, dt_gamma, max_steps, cascade, Hh)
        self.alive = [torch.arange(N, dtype=torch.int32, device="cuda"), torch.full((N,), -7, dtype=torch.int32, device="cuda")]
        self.count = [torch.full((1,), N, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")]
        self.rays_t = dev(near.copy())
        self.steps = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.total = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.table = torch.full((N, 3), -1, dtype=torch.int32, device="cuda")
        self.ws = torch.zeros(N, device="cuda")
        self.depth = torch.zeros(N, device="cuda")
        self.image = torch.zeros((N, K), device="cuda")
        self.trans = torch.ones(N, device="cuda")
        self.cur, self.n_alive, self.K = 0, N, K

    def march(self, n_step, fill=float("nan")):
        from gpu_util import call, host
        bound, dt_gamma, max_steps, cascade, Hh = self.geo
        M = self.n_alive * n_step
        # NaN-filled (unless a field is to run on the rows): whatever the round is to use, the marcher has to write
        self.xyzs = torch.full((M, 3), fill, device="cuda")
        self.deltas = torch.full((M, 2), float("nan"), device="cuda")
        c = self.cur
        call("lnh_lidar_march_rays", self.n_alive, n_step, self.N, self.count[c], self.alive[c], self.rays_t, self.steps,
             self.o, self.d, self.bits, bound, dt_gamma, max_steps, cascade, Hh, self.far, self.xyzs, self.deltas,
             self.table, self.total)
        return host(self.table).copy(), host(self.xyzs).copy(), host(self.deltas).copy()

    def composite(self, n_step, sig, feats):
        from gpu_util import call, dev, host
        c = self.cur
        call("lnh_lidar_composite_rays", self.n_alive, n_step, self.N, self.K, T_THRESH, self.count[c], self.alive[c],
             self.rays_t, self.table, dev(sig), dev(feats), self.deltas, self.xyzs, self.o, self.d, self.ws, self.depth,
             self.image, self.trans)
        marked = host(self.alive[c]).copy()
        call("lnh_alive_compact", self.n_alive, self.count[c], self.alive[c], self.alive[1 - c], self.count[1 - c])
        self.cur = 1 - c
        n = int(host(self.count[self.cur])[0])
        lst = host(self.alive[self.cur])[:n].copy()
        self.n_alive = n
        return marked, lst


@pytest.mark.parametrize("n_step", [1, 8, 24, 64])
@pytest.mark.parametrize("cascade,bound,dt_gamma", [(1, 1.0, 0.0), (2, 2.0, 1 / 128)])
def test_rounds_walk_the_training_lattice_bit_for_bit(cascade, bound, dt_gamma, n_step):
    """1. Per ray, the xyzs / deltas of all rounds concatenated ARE the samples c_oracle.march_rays_train (noises = 0) gives
    that ray, and the per-round counts add up to its count — for rounds of 1, 8, 24 and 64 samples, rays that miss the box
    and rays with far < near included.  The compositor gets sigma = 0: no ray ever saturates, a ray ends only where the walk
    does."""
    bits, Hh = _scene(cascade)
    N = 260
    o, d, wn, wf = _rays(N, bound, 7)
    big = N * 1024
    wx, _, wdl, wr, wc = c_oracle.march_rays_train(o, d, bits, bound, dt_gamma, 1024, cascade, Hh, big, wn, wf,
                                                   np.zeros(N, np.float32))
    assert int(wc[0]) > 20 * N and int((wr[:, 2] == 0).sum()) >= 2 * (N // 13)
    L = _Loop(o, d, wn, wf, bits, bound, cascade, Hh, dt_gamma)
    got_x, got_d = [[] for _ in range(N)], [[] for _ in range(N)]
    rounds, cap = 0, math.ceil(1024 / n_step)
    while L.n_alive > 0:
        assert rounds < cap, "the loop spins"
        n_alive = L.n_alive
        table, xyzs, deltas = L.march(n_step)
        assert (table[n_alive:] == 0).all()                                  # rows beyond the alive count are empty
        np.testing.assert_array_equal(table[:n_alive, 1], np.arange(n_alive) * n_step)
        for n in range(n_alive):
            rid, off, cnt = (int(v) for v in table[n])
            assert 0 <= cnt <= n_step
            got_x[rid].append(xyzs[off:off + cnt])
            got_d[rid].append(deltas[off:off + cnt])
            assert (deltas[off + cnt:off + n_step] == 0).all()               # unfilled slots: delta == 0
        M = n_alive * n_step
        marked, lst = L.composite(n_step, np.zeros(M, np.float32), np.zeros((M, 2), np.float32))
        np.testing.assert_array_equal(lst, table[:n_alive, 0][table[:n_alive, 2] == n_step])   # short round = dead, in order
        rounds += 1
    order = np.argsort(wr[:, 0], kind="stable")
    for rid in range(N):
        _, b, k = (int(v) for v in wr[order[rid]])
        x = np.concatenate(got_x[rid]) if got_x[rid] else np.zeros((0, 3), np.float32)
        dl = np.concatenate(got_d[rid]) if got_d[rid] else np.zeros((0, 2), np.float32)
        assert x.shape[0] == k, (rid, x.shape[0], k)
        np.testing.assert_array_equal(x, wx[b:b + k])
        np.testing.assert_array_equal(dl, wdl[b:b + k])
    from gpu_util import host
    assert int(host(L.total)[0]) == int(wc[0])
    assert float(host(L.ws).max()) == 0.0 and float(host(L.trans).min()) == 1.0
    _say(f"lattice cascade {cascade} n_step {n_step}: {rounds} rounds, {int(wc[0])} samples")


def test_max_steps_retires_a_ray_with_the_resume_mark():
    """A coarse cap (max_steps = 40 sets dt_min; a ray cannot hold more lattice points than that, but with everything occupied
    some hold exactly 40): counts still add up to the oracle's, nobody outlives ceil(max_steps / n_step) rounds, and a retired
    ray carries +inf in rays_t."""
    from gpu_util import host
    bits = np.full(128 ** 3 // 8, 255, np.uint8)
    N, n_step, max_steps = 64, 8, 40
    o, d, wn, wf = _rays(N, 1.0, 19)
    wx, _, wdl, wr, wc = c_oracle.march_rays_train(o, d, bits, 1.0, 0.0, max_steps, 1, 128, N * max_steps, wn, wf,
                                                   np.zeros(N, np.float32))
    assert int(wr[:, 2].max()) == max_steps
    L = _Loop(o, d, wn, wf, bits, 1.0, 1, 128, 0.0, max_steps=max_steps)
    rounds = 0
    while L.n_alive > 0:
        assert rounds < math.ceil(max_steps / n_step)
        M = L.n_alive * n_step
        L.march(n_step)
        L.composite(n_step, np.zeros(M, np.float32), np.zeros((M, 2), np.float32))
        rounds += 1
    order = np.argsort(wr[:, 0], kind="stable")
    np.testing.assert_array_equal(host(L.steps), wr[order, 2])
    assert np.isinf(host(L.rays_t)[wr[order, 2] > 0]).all()


def _composite_f64(state, table, n_alive, n_step, sig, feats, deltas, xyzs, o, d, steps_total, max_steps=1024):
    """float64 restatement of one compositor round: K channels, absolute depth, CARRIED transmittance, stop after the sample
    that takes T below the threshold; dead = stopped | short round | retired by the marcher.  Returns the marked list."""
    ws, depth, image, T = state
    marked = np.full(n_alive, -1, np.int64)
    for n in range(n_alive):
        rid, off, cnt = (int(v) for v in table[n])
        stopped = False
        for i in range(off, off + cnt):
            alpha = 1.0 - math.exp(-float(sig[i]) * float(deltas[i, 0]))
            w = alpha * T[rid]
            z = float(np.dot(xyzs[i].astype(np.float64) - o[rid].astype(np.float64), d[rid].astype(np.float64)))
            ws[rid] += w
            depth[rid] += w * z
            image[rid] += w * feats[i].astype(np.float64)
            T[rid] *= 1.0 - alpha
            if T[rid] < T_THRESH:
                stopped = True
                break
        dead = stopped or cnt < n_step or steps_total[rid] >= max_steps
        marked[n] = -1 if dead else rid
    return marked


@pytest.mark.parametrize("n_step", [8, 24, 100])
def test_compositor_rounds_vs_float64_restatement(n_step):
    """2. Random sigma / feats per round (some samples opaque: saturation inside a round, at its last sample, across rounds),
    K = 2: after EVERY round weights_sum / depth / image / carried T against the float64 restatement above, the marked list,
    the compacted list and the device count exactly.  Tolerance: what tests/test_raymarch_gpu.py grants the same kind of sum
    against its oracle, rtol 1e-5 / atol 1e-6.  n_step 8 / 24 / 100 = groups of 8 / 32 / 64 lanes (100: two chunks per round)."""
    from gpu_util import host
    bits, Hh = _scene(1)
    N = 300
    o, d, wn, wf = _rays(N, 1.0, 23)
    r = np.random.default_rng(100 + n_step)
    L = _Loop(o, d, wn, wf, bits, 1.0, 1, Hh, 0.0)
    state = (np.zeros(N), np.zeros(N), np.zeros((N, 2)), np.ones(N))
    rounds = worst = 0
    saturated = 0
    while L.n_alive > 0:
        assert rounds < math.ceil(1024 / n_step)
        n_alive = L.n_alive
        table, xyzs, deltas = L.march(n_step)
        M = n_alive * n_step
        sig = (r.random(M) * 12).astype(np.float32)
        sig[r.random(M) < 0.02] = 4000.0
        feats = r.random((M, 2)).astype(np.float32)
        marked, lst = L.composite(n_step, sig, feats)
        want = _composite_f64(state, table, n_alive, n_step, sig, feats, deltas, xyzs, o, d, host(L.steps))
        np.testing.assert_array_equal(marked[:n_alive], want)
        np.testing.assert_array_equal(lst, want[want >= 0])
        assert L.n_alive == int((want >= 0).sum())
        for got, ref in ((L.ws, state[0]), (L.depth, state[1]), (L.image, state[2]), (L.trans, state[3])):
            g = host(got).astype(np.float64)
            worst = max(worst, float(np.abs(g - ref).max()))
            np.testing.assert_allclose(g, ref, rtol=1e-5, atol=1e-6)
        saturated = int((state[3] < T_THRESH).sum())
        rounds += 1
    assert rounds >= 2 and saturated > N // 4 and float(state[0].max()) <= 1.0 + 1e-9
    _say(f"compositor n_step {n_step}: {rounds} rounds, {saturated} rays saturated, worst abs deviation {worst:.3e}")


# ------------------------------------------------------------------------------------------------ renderer
def _wall_net(fused_lidar=True, seed=0):
    """A seeded field with hard surfaces: the density row of the sigma net scaled up, so that the density is either
    negligible or opaque within a step or two (exp of a wide-ranged value), and the occupancy grid refreshed from it."""
    from lidarnerf.nerf.network import NeRFNetwork
    torch.manual_seed(seed)
    net = NeRFNetwork(encoding="hashgrid", desired_resolution=2048, bound=1, min_near=SCALE, min_near_lidar=SCALE,
                      density_thresh=10, cuda_ray=True, fused_lidar=fused_lidar)
    with torch.no_grad():
        net.encoder.embeddings.uniform_(-0.5, 0.5)
        net.sigma_net[1].weight[0] *= 200.0
    net = net.cuda().eval()
    torch.manual_seed(seed + 1)
    net.update_extra_state()
    return net


def _ring_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(n, generator=g) * 2 * np.pi
    o = torch.stack([0.6 * torch.cos(ang), 0.6 * torch.sin(ang), torch.zeros(n)], -1)
    target = (torch.rand(n, 3, generator=g) - 0.5) * 0.3
    d = torch.nn.functional.normalize(target - o, dim=-1)
    d[::97] = torch.tensor([0.0, 0.0, 1.0])   # straight up from the ring
    o[::89] += torch.tensor([0.0, 0.0, 3.0])  # outside the box, looking away or through it
    return o.cuda(), d.cuda()


def _existing_samples_and_field(net, o, d, fused_lidar):
    """What run_cuda's evaluation consumes: its marched samples and ITS OWN sigmas / feats on them (the same kernels)."""
    from lidarnerf import _hip, raymarching
    from lidarnerf.nerf import fused
    N = o.shape[0]
    nears, fars = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    _hip.call("lnh_lidar_march_prologue", o.data_ptr(), d.data_ptr(), net.aabb_infer.contiguous().data_ptr(), N,
              float(net.min_near_lidar), 81.0, nears.data_ptr(), fars.data_ptr(), None, None, 0)
    xyzs, dirs, deltas, rays = raymarching.march_rays_train(o, d, net.bound, net.density_bitfield, net.cascade, net.grid_size,
                                                            nears, fars, None, -1, False, 128, True, 0, 1024)
    M = xyzs.shape[0]
    if fused_lidar:
        assert fused.ragged_supported(net)
        sig, feats = fused.RaggedEvalField(net, d, M)(xyzs.contiguous(), rays, M)
    else:
        dens = net.density(xyzs)
        sig = dens["sigma"].float() * net.density_scale
        feats = net.color(xyzs, dirs, cal_lidar_color=True, mask=None, geo_feat=dens["geo_feat"]).float()
    return xyzs, deltas, rays, sig.float(), feats.float()


def _f64_ragged(xyzs, deltas, rays, sig, feats, o, d):
    """float64 composite (absolute depth, K = 2, stop after T < T_thresh) of ragged samples; also the index of the sample
    each ray stopped at (count - 1 when it never saturated, -1 without samples)."""
    xyzs, deltas, rays = xyzs.cpu().numpy().astype(np.float64), deltas.cpu().numpy().astype(np.float64), rays.cpu().numpy()
    sig, feats = sig.cpu().numpy().astype(np.float64), feats.cpu().numpy().astype(np.float64)
    o, d = o.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.float64)
    N = rays.shape[0]
    ws, depth, image, stop_at = np.zeros(N), np.zeros(N), np.zeros((N, 2)), np.full(N, -1)
    counts = np.zeros(N, np.int64)
    for rid, off, cnt in rays:
        counts[rid] = cnt
        if cnt == 0:
            continue
        sl = slice(off, off + cnt)
        alpha = 1.0 - np.exp(-sig[sl] * deltas[sl, 0])
        T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)])
        below = np.nonzero(T[1:] < T_THRESH)[0]
        last = int(below[0]) if below.size else cnt - 1
        w = alpha * T[:-1] * (np.arange(cnt) <= last)
        z = ((xyzs[sl] - o[rid]) * d[rid]).sum(-1)
        ws[rid], depth[rid], image[rid], stop_at[rid] = w.sum(), (w * z).sum(), (w[:, None] * feats[sl]).sum(0), last
    return ws, depth, image, stop_at, counts


def _rel(a, b):
    """largest deviation over the largest entry"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# 3./6.: the existing evaluation's deviation from a float64 composite of its own sigmas / feats (largest deviation over the
# largest entry), measured once on an MI355X on the rays of test 3, largest of the four (MLP build, field) cases:
#   depth_lidar 1.473e-07 (fp16; bf16 1.104e-07), image_lidar 2.283e-07 (fp16 modular; 1.991e-07 .. 2.278e-07 elsewhere),
#   weights_sum_lidar 1.873e-07 (fp16; bf16 1.788e-07).
# The bound for new-vs-existing is TWICE that: both paths composite identical samples with identical sigmas / feats, only
# the order of the float sums differs.  (Seen for new-vs-existing in the same run: 1.05e-07 / 2.76e-07 / 2.38e-07.)
EXISTING_VS_F64 = {"depth_lidar": 1.473e-7, "image_lidar": 2.283e-7, "weights_sum_lidar": 1.873e-7}
BOUND = {k: 2 * v for k, v in EXISTING_VS_F64.items()}


def _render(net, o, d, mdt, **kw):
    with torch.no_grad(), torch.autocast("cuda", dtype=mdt):
        out = net.render(o[None], d[None], cal_lidar_color=True, perturb=False, **kw)
    return {k: v.float().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("fused_lidar", [True, False], ids=["fused", "modular"])
@pytest.mark.parametrize("mdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_alive_evaluation_equals_the_existing_evaluation(mdt, fused_lidar):
    """3. + 4. + 5. on the wall scene, 3000 rays, fp16 / bf16 MLP builds, fused / modular field.

    3. depth_lidar / image_lidar / weights_sum_lidar of run_cuda_alive vs run_cuda as it is, within BOUND (above: twice the
       existing path's own deviation from float64, which this test re-measures and prints); rays without samples are zero on
       both.
    4. the new path shades strictly fewer samples than the existing path marches; the sample buffer is at most
       N * n_step_max * 8 * 4 bytes (the per-ray half of 4. is the next test).
    5. a second call gives the same bits."""
    from lidarnerf import raymarching
    net = _wall_net(fused_lidar)
    N = 3000
    o, d = _ring_rays(N, 5)
    old = _render(net, o, d, mdt)
    new = _render(net, o, d, mdt, alive_march=True)
    stats = dict(net.alive_stats)
    again = _render(net, o, d, mdt, alive_march=True)
    with torch.no_grad(), torch.autocast("cuda", dtype=mdt):
        xyzs, deltas, rays, sig, feats = _existing_samples_and_field(net, o, d, fused_lidar)
    ws, depth, image, stop_at, counts = _f64_ragged(xyzs, deltas, rays, sig, feats, o, d)
    ref = {"depth_lidar": depth, "image_lidar": image, "weights_sum_lidar": ws}
    saturated = int(((stop_at >= 0) & (stop_at < counts - 1)).sum())
    assert saturated > N // 3 and int((counts == 0).sum()) > 0, (saturated, int((counts == 0).sum()))
    for k in BOUND:
        dev_old, dev_new, diff = _rel(old[k].reshape(ref[k].shape), ref[k]), _rel(new[k].reshape(ref[k].shape), ref[k]), \
            _rel(new[k], old[k])
        _say(f"{k} [{'fused' if fused_lidar else 'modular'}, {mdt}]: existing vs f64 {dev_old:.3e}, new vs f64 {dev_new:.3e}, "
             f"new vs existing {diff:.3e} (bound {BOUND[k]:.1e})")
    for k in BOUND:
        assert _rel(new[k], old[k]) <= BOUND[k], (k, _rel(new[k], old[k]))
        assert (new[k].reshape(N, -1)[counts == 0] == 0).all() and (old[k].reshape(N, -1)[counts == 0] == 0).all()
        np.testing.assert_array_equal(new[k], again[k])                                             # 5.
    # 4.
    marched = int(counts.sum())
    assert stats["samples"] < marched, (stats["samples"], marched)
    assert stats["sample_buffer_bytes"] <= N * raymarching.ALIVE_N_STEP_MAX * 8 * 4
    assert stats["rounds"] == len(stats["n_steps"]) <= raymarching.alive_max_rounds(1024)
    _say(f"early stop: {stats['samples']} samples shaded vs {marched} marched, rounds {stats['rounds']}, n_step "
         f"{stats['n_steps']}, buffer {stats['sample_buffer_bytes']} B vs {marched * 8 * 4} B")


def test_every_ray_stops_within_a_round_of_its_saturation():
    """4., per ray, through the raw loop with the renderer's schedule: a ray whose existing-path composite stopped at sample k
    (0-based) has been shaded for fewer than (k + 1) + n_step samples, n_step the largest round used."""
    from lidarnerf import raymarching
    from lidarnerf.nerf import fused
    from gpu_util import host
    net = _wall_net(True)
    N = 2000
    o, d = _ring_rays(N, 9)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        xyzs, deltas, rays, sig, feats = _existing_samples_and_field(net, o, d, True)
        _, _, _, stop_at, counts = _f64_ragged(xyzs, deltas, rays, sig, feats, o, d)
        fars = torch.empty(N, device="cuda")
        nears = torch.empty(N, device="cuda")
        from lidarnerf import _hip
        _hip.call("lnh_lidar_march_prologue", o.data_ptr(), d.data_ptr(), net.aabb_infer.contiguous().data_ptr(), N,
                  float(net.min_near_lidar), 81.0, nears.data_ptr(), fars.data_ptr(), None, None, 0)
        L = _Loop(host(o), host(d), host(nears), host(fars), host(net.density_bitfield), 1.0, 1, 128, 0.0)
        shaded = np.zeros(N, np.int64)
        n_max = 0
        while L.n_alive > 0:
            n_alive = L.n_alive
            n_step = raymarching.alive_n_step(n_alive, N)
            n_max = max(n_max, n_step)
            table, _, _ = L.march(n_step, fill=0.0)
            M = n_alive * n_step
            s, f = fused.RaggedEvalField(net, d, M)(L.xyzs, L.table, M)
            np.add.at(shaded, table[:n_alive, 0], table[:n_alive, 2])
            L.composite(n_step, host(s), host(f))
    has = counts > 0
    assert (shaded[has] < stop_at[has] + 1 + n_max).all()
    assert (shaded <= counts).all() and int(shaded.sum()) < int(counts.sum())
    # the field on a round's samples is the field on the same samples of the full march: the outputs agree as in test 3
    ws = host(L.ws)
    want, _, _, _, _ = _f64_ragged(xyzs, deltas, rays, sig, feats, o, d)
    assert _rel(ws, want) <= 1e-5


def test_staged_frames_take_the_switch_and_training_ignores_it():
    """6. render(staged=True) over more rays than max_ray_batch: the new path chunk by chunk vs the same call on the existing
    path, BOUND as above; the module attribute selects it as well; in .train() mode the switch changes nothing — same
    outputs bit for bit, same autograd node, the same table gradient to the run-to-run spread of the training path."""
    net = _wall_net(True)
    N = 2500
    o, d = _ring_rays(N, 13)
    old = _render(net, o, d, torch.float16, staged=True, max_ray_batch=1024)
    net.alive_stats_log = []
    new = _render(net, o, d, torch.float16, staged=True, max_ray_batch=1024, alive_march=True)
    assert len(net.alive_stats_log) == 3 and [s["rays"] for s in net.alive_stats_log] == [1024, 1024, 452]
    net.alive_march = True
    net.alive_stats = None
    attr = _render(net, o, d, torch.float16, staged=True, max_ray_batch=1024)
    assert net.alive_stats is not None
    off = _render(net, o, d, torch.float16, staged=True, max_ray_batch=1024, alive_march=False)   # the keyword wins
    net.alive_march = False
    for k in ("depth_lidar", "image_lidar"):
        _say(f"staged {k}: new vs existing {_rel(new[k], old[k]):.3e} (bound {BOUND[k]:.1e})")
        assert _rel(new[k], old[k]) <= BOUND[k]
        np.testing.assert_array_equal(new[k], attr[k])
        np.testing.assert_array_equal(off[k], old[k])
    # training mode
    net.train()
    net.alive_stats = None
    res = []
    for flag in (None, True):
        net.zero_grad()
        torch.manual_seed(3)
        with torch.autocast("cuda", dtype=torch.float16):
            kw = {} if flag is None else {"alive_march": flag}
            out = net.render(o[None, :512], d[None, :512], cal_lidar_color=True, perturb=False, force_all_rays=True, **kw)
        assert out["depth_lidar"].grad_fn is not None
        (out["depth_lidar"].sum() + out["image_lidar"].sum()).backward()
        res.append((out["depth_lidar"].detach().clone(), out["image_lidar"].detach().clone(),
                    type(out["depth_lidar"].grad_fn).__name__, net.encoder.embeddings.grad.detach().clone()))
    assert net.alive_stats is None
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    # the same node, so the same gradient — up to what two runs of the SAME training call differ by: the training marcher
    # hands out sample rows in arrival order, and the fp16 table gradient (11 significant bits per partial sum) is added up
    # in that order.  1e-3 of the gradient's norm is a handful of such roundings; a different graph would be off by O(1).
    ga, gb = res[0][3].double(), res[1][3].double()
    rel = float((ga - gb).norm() / ga.norm())
    _say(f"training gradient, switch on vs off: relative difference {rel:.3e}")
    assert float(gb.abs().sum()) > 0 and rel < 1e-3
