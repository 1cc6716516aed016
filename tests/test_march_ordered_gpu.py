"""lnh_march_rays_train_ordered (csrc/raymarch.hip: count per ray, one-workgroup integer scan, write per ray) — the whole
output (sample arrays, ray table, counter) bit for bit against the serial C oracle, which hands out rows in ray order
natively; per ray against the arrival-order kernel; the overflow rule as a function of the inputs alone; run to run and
through a captured graph; the argument refusals of lnh_march_rays_train."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle

pytestmark = pytest.mark.gpu
HH = 128
N_MAX = 4099  # more rays than one tile of the scan (4096)
NAMES = ("xyzs", "dirs", "deltas", "rays", "counter")


@functools.lru_cache(maxsize=None)
def _bits(cascade, kind="random"):
    """Occupancy bitfield of cascade * 128^3 cells: about 30 % set bits (fixed seed), none, or all."""
    n = cascade * HH ** 3
    if kind == "empty":
        return np.zeros(n // 8, np.uint8)
    if kind == "full":
        return np.full(n // 8, 0xFF, np.uint8)
    cells = np.random.default_rng(101).random(n) < 0.3
    return np.packbits(cells, bitorder="little")  # (cell i is bit i & 7 of byte i >> 3)


@functools.lru_cache(maxsize=None)
def _rays(cascade, bound):
    """The rays of tests/test_raymarch_gpu.py (a bundle from inside the -x face), their box ranges and start jitters."""
    r = np.random.default_rng(7)
    o = (r.standard_normal((N_MAX, 3)) * 0.05 + np.array([-0.8 * bound, 0.1, 0.0])).astype(np.float32)
    d = r.standard_normal((N_MAX, 3)).astype(np.float32)
    d[:, 0] = np.abs(d[:, 0]) + 0.7
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = c_oracle.near_far_from_aabb(o, d, aabb, 0.05)
    return o, d, nears, fars, r.random(N_MAX, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _want(N, cascade, bound, dt_gamma, noise, kind="random", max_steps=1024):
    """Inputs and the oracle's outputs with room for every sample (M = total + 64: a tail no ray owns), computed once."""
    o, d, nears, fars, noises = (a[:N] for a in _rays(cascade, bound))
    if not noise:
        noises = np.zeros(N, np.float32)
    bits = _bits(cascade, kind)
    total = int(c_oracle.march_rays_train(o, d, bits, bound, dt_gamma, max_steps, cascade, HH, 1, nears, fars, noises)[4][0])
    M = total + 64
    out = c_oracle.march_rays_train(o, d, bits, bound, dt_gamma, max_steps, cascade, HH, M, nears, fars, noises)
    for a in out:
        a.setflags(write=False)  # (shared among the tests: left unchanged)
    return (o, d, bits, nears, fars, noises), M, out


def _march(name, inputs, cascade, bound, dt_gamma, max_steps, M):
    """One launch of entry point `name` into cleared buffers of M rows: (xyzs, dirs, deltas, rays, counter) on the device."""
    from gpu_util import call, dev
    o, d, bits, nears, fars, noises = inputs
    N = o.shape[0]
    out = (torch.zeros((M, 3), device="cuda"), torch.zeros((M, 3), device="cuda"), torch.zeros((M, 2), device="cuda"),
           torch.zeros((N, 3), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))
    call(name, dev(o), dev(d), dev(bits), bound, dt_gamma, max_steps, N, cascade, HH, M, dev(nears), dev(fars), *out,
         dev(noises))
    torch.cuda.synchronize()
    return out


def _assert_bits(got, want):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=name)


# ------------------------------------------------------------------------------------------------ 1. the C oracle
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("dt_gamma", [0.0, 1 / 128])
@pytest.mark.parametrize("cascade,bound", [(1, 1.0), (2, 2.0)])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 1000, 4099])
def test_whole_output_equals_the_oracle(N, cascade, bound, dt_gamma, noise):
    inputs, M, want = _want(N, cascade, bound, dt_gamma, noise)
    got = _march("lnh_march_rays_train_ordered", inputs, cascade, bound, dt_gamma, 1024, M)
    _assert_bits(got, want)
    assert want[4][1] == N and want[4][0] == want[3][:, 2].sum() and (N < 16 or want[4][0] > 10 * N)


def test_empty_grid():
    inputs, M, want = _want(1000, 1, 1.0, 0.0, True, kind="empty")
    got = _march("lnh_march_rays_train_ordered", inputs, 1, 1.0, 0.0, 1024, M)
    _assert_bits(got, want)
    assert got[4].tolist() == [0, 1000] and int(got[3][:, 1:].abs().sum()) == 0


def test_full_grid_where_max_steps_binds_on_every_ray():
    inputs, M, want = _want(1000, 1, 1.0, 0.0, True, kind="full", max_steps=16)
    assert (want[3][:, 2] == 16).all()
    got = _march("lnh_march_rays_train_ordered", inputs, 1, 1.0, 0.0, 16, M)
    _assert_bits(got, want)
    assert got[4].tolist() == [16000, 1000]


# ------------------------------------------------------------------------------------------------ 2. the existing kernel
@pytest.mark.parametrize("N,cascade,bound,dt_gamma", [(4099, 1, 1.0, 0.0), (1000, 2, 2.0, 1 / 128)])
def test_per_ray_equals_the_arrival_order_kernel(N, cascade, bound, dt_gamma):
    inputs, M, _ = _want(N, cascade, bound, dt_gamma, True)
    new = [t.cpu().numpy() for t in _march("lnh_march_rays_train_ordered", inputs, cascade, bound, dt_gamma, 1024, M)]
    old = [t.cpu().numpy() for t in _march("lnh_march_rays_train", inputs, cascade, bound, dt_gamma, 1024, M)]
    np.testing.assert_array_equal(new[3][:, 0], np.arange(N))
    cnt = new[3][:, 2].astype(np.int64)
    np.testing.assert_array_equal(new[3][:, 1], np.cumsum(cnt) - cnt)  # exclusive prefix sum in ray order
    np.testing.assert_array_equal(new[4], old[4])
    by_id = old[3][np.argsort(old[3][:, 0])]
    np.testing.assert_array_equal(by_id[:, 0], np.arange(N))
    np.testing.assert_array_equal(by_id[:, 2], new[3][:, 2])
    for n in range(N):
        a, b, k = int(new[3][n, 1]), int(by_id[n, 1]), int(cnt[n])
        for x, y in zip(new[:3], old[:3]):
            assert np.array_equal(x[a:a + k].view(np.uint32), y[b:b + k].view(np.uint32)), n


# ------------------------------------------------------------------------------------------------ 3. overflow
def test_overflow_drops_a_set_the_inputs_decide():
    N, cascade, bound, dt_gamma = 4099, 1, 1.0, 0.0
    inputs, M_all, want = _want(N, cascade, bound, dt_gamma, True)
    M = int(want[4][0]) // 2
    got = [t.cpu().numpy() for t in _march("lnh_march_rays_train_ordered", inputs, cascade, bound, dt_gamma, 1024, M)]
    np.testing.assert_array_equal(got[3], want[3])  # the table and the counter of the unconstrained run
    np.testing.assert_array_equal(got[4], want[4])
    cnt = want[3][:, 2].astype(np.int64)
    off = np.cumsum(cnt) - cnt
    dropped = off + cnt > M
    assert dropped.any() and (~dropped).any() and (cnt[dropped] > 0).any()
    owned = np.zeros(M, bool)
    for n in np.nonzero(~dropped)[0]:
        owned[off[n]:off[n] + cnt[n]] = True
    assert (cnt[~dropped] > 0).any() and owned.any() and not owned.all()  # (rows in front of M that a dropped ray would own)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g[owned].view(np.uint32), w[:M][owned].view(np.uint32))  # kept rays: the unconstrained bits
        assert not g[~owned].view(np.uint32).any()                                     # every other row as it was cleared
    # ... and the oracle with the same M agrees on everything
    o, d, bits, nears, fars, noises = inputs
    _assert_bits(got, c_oracle.march_rays_train(o, d, bits, bound, dt_gamma, 1024, cascade, HH, M, nears, fars, noises))


# ------------------------------------------------------------------------------------------------ 4. run to run
def test_two_launches_and_two_replays_give_the_same_bits():
    from gpu_util import call, dev
    from lidarnerf import _hip
    N, cascade, bound, dt_gamma = 4099, 1, 1.0, 0.0
    inputs, M, want = _want(N, cascade, bound, dt_gamma, True)
    a = _march("lnh_march_rays_train_ordered", inputs, cascade, bound, dt_gamma, 1024, M)
    b = _march("lnh_march_rays_train_ordered", inputs, cascade, bound, dt_gamma, 1024, M)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # one captured graph (clear, march) replayed twice
    o, d, bits, nears, fars, noises = (dev(t) for t in inputs)
    buf = torch.empty(M * 8, device="cuda")
    outs = (buf[:M * 3].view(M, 3), buf[M * 3:M * 6].view(M, 3), buf[M * 6:].view(M, 2),
            torch.empty((N, 3), dtype=torch.int32, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda"))

    def launch():
        _hip.zero_regions([buf, outs[3], outs[4]])  # (a kernel: zero fills of a captured step are never memset nodes)
        call("lnh_march_rays_train_ordered", o, d, bits, bound, dt_gamma, 1024, N, cascade, HH, M, nears, fars, *outs, noises)

    launch()  # (every kernel's code is loaded before anything is captured)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    replays = []
    for _ in range(2):
        for t in (buf, outs[3], outs[4]):
            t.fill_(-1)  # (what the replay must overwrite)
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in outs])
    for x, y, z in zip(a, *replays):
        assert torch.equal(x, y) and torch.equal(x, z)
    _assert_bits(replays[1], want)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_are_those_of_the_arrival_order_entry_point():
    from lidarnerf import _hip
    L = _hip.lib()
    N, M = 16, 64
    f = lambda *shape: torch.full(shape, 7.0, device="cuda")
    o, d, nears, fars, noises = f(N, 3), f(N, 3), f(N), f(N), f(N)
    bits = torch.zeros(HH ** 3 // 8, dtype=torch.uint8, device="cuda")
    outs = [f(M, 3), f(M, 3), f(M, 2), torch.full((N, 3), 7, dtype=torch.int32, device="cuda"),
            torch.full((2,), 7, dtype=torch.int32, device="cuda")]
    ptrs = [o, d, bits, nears, fars] + outs + [noises]

    def rc(name, n=N, C=1, H=HH, max_steps=1024, null=None):
        p = [None if i == null else t.data_ptr() for i, t in enumerate(ptrs)]
        return getattr(L, name)(p[0], p[1], p[2], 1.0, 0.0, max_steps, n, C, H, M, p[3], p[4], p[5], p[6], p[7], p[8], p[9],
                                p[10], _hip.stream())

    bad = [dict(null=i) for i in range(len(ptrs))] + [dict(C=0), dict(C=9), dict(H=0), dict(H=1025), dict(max_steps=0)]
    for kw in bad:
        assert rc("lnh_march_rays_train_ordered", **kw) == -1 and b"march_rays_train_ordered" in L.lnh_last_error(), kw
        assert rc("lnh_march_rays_train", **kw) == -1, kw
    assert rc("lnh_march_rays_train_ordered", n=0) == 0 == rc("lnh_march_rays_train", n=0)
    torch.cuda.synchronize()
    for t in [o, d, nears, fars, noises] + outs:  # nothing launched, nothing written
        assert bool((t == 7).all())
