"""HIP hash-grid encoder vs the CPU oracle, through the C ABI (lnh_grid_*)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, grid_ref

pytestmark = pytest.mark.gpu

H, L, CH = 16, 16, 2
PLS = grid_ref.per_level_scale(32768, H, L)
S = float(np.log2(PLS))
OFF = grid_ref.make_offsets(3, L, PLS, H, 19)


def _points(B, seed, D=3):
    r = np.random.default_rng(seed)
    x = r.random((B, D), dtype=np.float32)
    x[0] = 0
    x[1] = 1
    x[2, 0] = 1.0000001
    x[3, 1] = -1e-7
    x[4] = 0.5
    return x


def _ray_points(n_rays, T, seed):
    """Consecutive samples along rays (exercises the wave run-merge in backward)."""
    r = np.random.default_rng(seed)
    o = r.random((n_rays, 1, 3), dtype=np.float32) * 0.2 + 0.4
    d = r.standard_normal((n_rays, 1, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.linspace(0.005, 0.45, T, dtype=np.float32)[None, :, None]
    return np.clip(o + d * t, 0, 1).reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("gridtype,align,D", [(0, False, 3), (1, False, 3), (0, True, 3), (0, False, 2), (0, False, 4)])
def test_corner_indices_bit_exact(gridtype, align, D):
    from gpu_util import call, dev, host
    x = _points(4099, 1, D)
    off = grid_ref.make_offsets(D, L, PLS, H, 19, align_corners=align)
    want = c_oracle.grid_indices(x, off, CH, S, H, gridtype, align)
    xd = dev(x)
    out = torch.empty((L, x.shape[0], 1 << D), dtype=torch.int32, device="cuda")
    offh = torch.from_numpy(off)
    call("lnh_grid_corner_indices", xd, offh, out, x.shape[0], D, CH, L, S, H, gridtype, int(align))
    np.testing.assert_array_equal(host(out).view(np.uint32), want)


def test_corner_indices_full_size_properties():
    """BASELINE size (4096 rays x 832 samples): every index in range, dense levels match the closed form."""
    from gpu_util import call, dev, host
    B = 4096 * 832
    x = torch.rand((B, 3), device="cuda")
    out = torch.empty((L, B, 8), dtype=torch.int32, device="cuda")
    call("lnh_grid_corner_indices", x, torch.from_numpy(OFF), out, B, 3, CH, L, S, H, 0, 0)
    rows = np.diff(OFF)
    for l in range(L):
        o = out[l].to(torch.int64) & 0xFFFFFFFF
        assert int(o.max()) < rows[l] * CH and int(o.min()) >= 0
    # level 0 is dense: row = x + y*R + z*R^2 with R = 17, corner 0
    sc, res = c_oracle.grid_level(0, S, H)
    pg = torch.floor(x * float(sc) + 0.5).to(torch.int64)
    want = (pg[:, 0] + pg[:, 1] * (res + 1) + pg[:, 2] * (res + 1) ** 2) * CH
    # x*scale+0.5 is one fma in the kernel; the torch expression above rounds twice -> allow the rare floor flip
    mism = (out[0, :, 0].to(torch.int64) != want).float().mean().item()
    assert mism < 1e-4
    # sample check against the oracle
    sel = torch.randint(0, B, (2048,), device="cuda")
    want_s = c_oracle.grid_indices(host(x[sel]), OFF, CH, S, H)
    np.testing.assert_array_equal(host(out[:, sel]).view(np.uint32), want_s)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [1, 2, 4, 8])
def test_forward(dt, C):
    from gpu_util import call, dev, host
    if dt == torch.float16 and C == 1:
        pytest.skip("reference forces fp32 for odd C (grid.py:54-57)")
    x = _points(3001, 2)
    r = np.random.default_rng(0)
    nd = np.float32 if dt == torch.float32 else np.float16
    emb = (r.random((int(OFF[-1]), C), dtype=np.float32) * 2 - 1).astype(nd)
    want, _ = c_oracle.grid_forward(x, emb, OFF, S, H)
    out = torch.empty((L, x.shape[0], C), dtype=dt, device="cuda")
    call("lnh_grid_encode_forward", dev(x), dev(emb), torch.from_numpy(OFF), out, x.shape[0], 3, C, L, S, H, None, 0, 0,
         0, 0 if dt == torch.float32 else 1)
    got = host(out)
    if dt == torch.float32:
        # same fma chain in the same corner order: bit exact
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("interp,gridtype,align", [(1, 0, False), (0, 1, False), (0, 0, True)])
def test_forward_variants_and_dydx(interp, gridtype, align):
    from gpu_util import call, dev, host
    x = _points(1500, 5)
    off = grid_ref.make_offsets(3, L, PLS, H, 19, align_corners=align)
    emb = np.random.default_rng(3).standard_normal((int(off[-1]), CH)).astype(np.float32)
    want, wdy = c_oracle.grid_forward(x, emb, off, S, H, gridtype, align, interp, calc_dy_dx=True)
    out = torch.empty((L, x.shape[0], CH), device="cuda")
    dy = torch.empty((x.shape[0], L, 3, CH), device="cuda")
    call("lnh_grid_encode_forward", dev(x), dev(emb), torch.from_numpy(off), out, x.shape[0], 3, CH, L, S, H, dy,
         gridtype, int(align), interp, 0)
    np.testing.assert_array_equal(host(out), want)
    np.testing.assert_allclose(host(dy), wdy, rtol=1e-5, atol=1e-4)
    # input backward
    g = np.random.default_rng(4).standard_normal((L, x.shape[0], CH)).astype(np.float32)
    ge = torch.zeros((int(off[-1]), CH), device="cuda")
    gi = torch.zeros((x.shape[0], 3), device="cuda")
    call("lnh_grid_encode_backward", dev(g), dev(x), None, torch.from_numpy(off), ge, x.shape[0], 3, CH, L, S, H, dy, gi,
         gridtype, int(align), interp, 0)
    np.testing.assert_allclose(host(gi), c_oracle.grid_input_backward(g, wdy), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["random", "rays"])
def test_backward(dt, kind):
    from gpu_util import call, dev, host
    x = _points(5000, 7) if kind == "random" else _ray_points(24, 256, 7)
    B = x.shape[0]
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(8).standard_normal((L, B, CH)) * 0.1).astype(nd)
    rows = int(OFF[-1])
    want = c_oracle.grid_backward(g, x, OFF, rows, S, H)
    ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
    call("lnh_grid_encode_backward", dev(g), dev(x), None, torch.from_numpy(OFF), ge, B, 3, CH, L, S, H, None, None, 0, 0,
         0, 0 if dt == torch.float32 else 1)
    got = host(ge).astype(np.float64)
    if dt == torch.float32:
        # atomics: order-dependent fp32 sums vs the order-free float64 oracle
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    else:
        # fp16 accumulation in the table (packed fp16 atomics): error grows with the number of addends per cell
        np.testing.assert_allclose(got, want, rtol=2e-2, atol=2e-2)
    # untouched cells stay exactly zero
    assert np.all(got[want == 0] == 0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["random", "rays", "same_cell", "tiny"])
def test_backward_bucketed(dt, kind):
    """lnh_grid_encode_backward_ws (no HBM atomics) must give the same table as the oracle's order-free sum."""
    from gpu_util import call, dev, host
    from lidarnerf import _hip
    if kind == "random":
        x = _points(5000, 7)
    elif kind == "rays":
        x = _ray_points(24, 256, 7)
    elif kind == "tiny":  # fewer points than a wave, one of them outside the grid
        x = np.random.default_rng(9).random((3, 3), dtype=np.float32)
        x[1] = [1.5, 0.2, 0.3]
    else:  # adversarial: every point in two cells -> their buckets overflow the pool, the excess takes the spill list
        x = (np.random.default_rng(1).random((20000, 3), dtype=np.float32) * 1e-6 + 0.3).astype(np.float32)
        x[::2] += np.float32(0.11)  # break the runs so the wave merge cannot collapse everything
    B = x.shape[0]
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(8).standard_normal((L, B, CH)) * 0.1).astype(nd)
    rows = int(OFF[-1])
    want = c_oracle.grid_backward(g, x, OFF, rows, S, H)
    code = 0 if dt == torch.float32 else 1
    offh = torch.from_numpy(OFF)
    need = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
    call("lnh_grid_encode_backward_ws", dev(g), dev(x), offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, need)
    got = host(ge).astype(np.float64)
    if dt == torch.float32:
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    else:  # exact fixed-point accumulation (pool and spill alike), ONE rounding to fp16 per touched row
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-3 * max(1.0, np.abs(want).max() / 10))
    assert np.all(got[want == 0] == 0)
    # too-small workspace is an error, not silent corruption
    with pytest.raises(RuntimeError, match="workspace too small"):
        call("lnh_grid_encode_backward_ws", dev(g), dev(x), offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, 1024)

@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("pattern", ["sprinkle30", "sprinkle70", "tail", "both", "all_zero"])
def test_backward_bucketed_with_zero_gradient_samples(dt, pattern):
    """Samples whose upstream gradient is exactly zero (everything behind a learned surface; sprinkled ones in a noisy field):
    within three lanes of a sample that has a gradient they stay silent members of its run, elsewhere they are dropped before
    the pool (profiles/r05_reduce_drift.txt) — either way the table is the oracle's, bit-reproducibly.  Ray-ordered points, so
    that runs exist on the coarse and middle levels."""
    from gpu_util import call, dev, host
    from lidarnerf import _hip
    n_rays, T = 48, 256
    x = _ray_points(n_rays, T, 11)
    B = x.shape[0]
    nd = np.float32 if dt == torch.float32 else np.float16
    r = np.random.default_rng(21)
    g = (r.standard_normal((L, B, CH)) * 0.1).astype(nd)
    keep = np.ones((n_rays, T), bool)
    if pattern in ("sprinkle30", "both"):
        keep &= r.random((n_rays, T)) >= 0.3
    if pattern == "sprinkle70":
        keep &= r.random((n_rays, T)) >= 0.7
    if pattern in ("tail", "both"):
        keep[:, T - 100:] = False
    if pattern == "all_zero":
        keep[:] = False
    g *= keep.reshape(1, B, 1).astype(nd)
    g[3, ::5] = 0  # ... and zeros that differ from level to level (a sample may be silent on one level only)
    rows = int(OFF[-1])
    want = c_oracle.grid_backward(g, x, OFF, rows, S, H)
    code = 0 if dt == torch.float32 else 1
    offh = torch.from_numpy(OFF)
    need = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
        call("lnh_grid_encode_backward_ws", dev(g), dev(x), offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, need)
        outs.append(ge)
    assert torch.equal(outs[0], outs[1])
    _check_table(host(outs[0]).astype(np.float64), want, dt)
    if pattern == "all_zero":
        assert float(outs[0].abs().max()) == 0.0


def _plan(B, level, code):
    """(buckets of the level, pool slots per bucket, rows per bucket, entries per reduce slice) of the workspace plan."""
    from lidarnerf import _hip
    out = np.zeros(4, dtype=np.uint32)
    rc = _hip.lib().lnh_grid_backward_plan_info(torch.from_numpy(OFF).data_ptr(), B, 3, CH, L, S, H, 0, 0, code, level,
                                                out.ctypes.data)
    assert rc == 0
    return [int(v) for v in out]


def _run_bucketed(x, g, dt, times=1):
    from gpu_util import call, dev, host
    from lidarnerf import _hip
    B, rows = x.shape[0], int(OFF[-1])
    code = 0 if dt == torch.float32 else 1
    offh = torch.from_numpy(OFF)
    need = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    gd, xd = dev(g), dev(x)
    outs = []
    for _ in range(times):
        ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
        ws.random_(0, 255)  # the workspace content before a call is irrelevant
        call("lnh_grid_encode_backward_ws", gd, xd, offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, need)
        outs.append(ge)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])  # integer accumulation: bit-reproducible whatever the arrival order
    return host(outs[0]).astype(np.float64)


def _check_table(got, want, dt, untouched=None):
    """`untouched`: the rows no point reaches, when the caller knows them.  Without it the oracle's exact zeros stand in — which
    is only right while no contribution is small enough for the oracle's per-contribution fp16 rounding (the reference's
    __half2 atomicAdd operand) to flush it to zero: the bucketed path keeps such a contribution in its 2^-24 fixed-point
    sum and may round the row to the smallest subnormals instead (seen at 700 K points: 2.4e-7 against 0)."""
    if dt == torch.float32:
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5)
    else:
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-3 * max(1.0, np.abs(want).max() / 10))
    if untouched is None:
        untouched = want == 0
    assert np.all(got[untouched] == 0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_backward_bucketed_overflow_by_a_few(dt):
    """A hashed level's bucket receives a handful of entries more than its pool holds (the round-1 flake: 1508 entries
    against 1504 slots): the excess goes through the spill list into the same integer sum — equal to the oracle and
    bit-identical run to run.  The input is built from the plan: random points + points alternating between two cells
    (alternating, so the wave run-merge cannot collapse them), as many as it takes to overflow by 1..8 entries."""
    code = 0 if dt == torch.float32 else 1
    B, level = 12288, 10
    nb, cap, brows, _ = _plan(B, level, code)
    assert nb == 64
    r = np.random.default_rng(11)
    base = r.random((B, 3), dtype=np.float32)
    cells = np.array([[0.3, 0.3, 0.3], [0.41, 0.41, 0.41]], dtype=np.float32)
    idx = c_oracle.grid_indices(base, OFF, CH, S, H)[level] // CH          # [B, 8] level-local rows
    cidx = c_oracle.grid_indices(cells, OFF, CH, S, H)[level] // CH        # [2, 8]

    def entry_buckets(ix):
        """Pool entries of points with corner rows ix [n, 8] (grid_pool.h, "pool entries"): one entry per x-neighbour pair of
        corners (2p, 2p + 1) in the bucket of the first row, plus one in the bucket of the second row when the rows differ
        in more than 7 low bits (r0 ^ r1 = 2^(t+1) - 1 with t >= 7: the pair travels as two singles).  -> (point, bucket)."""
        r0, r1 = ix[:, 0::2], ix[:, 1::2]
        t = np.array([[bin(int(v)).count("1") - 1 for v in row] for row in (r0 ^ r1)])
        pts = np.repeat(np.arange(ix.shape[0]), 4)
        p_all, b_all = [pts], [(r0 >> 13).ravel()]
        sel = (t >= 7).ravel()
        p_all.append(pts[sel])
        b_all.append((r1 >> 13).ravel()[sel])
        return np.concatenate(p_all), np.concatenate(b_all)

    pts, bks = entry_buckets(idx)
    onehot = np.zeros((B + 1, nb), dtype=np.int64)
    np.add.at(onehot[1:], (pts, bks), 1)
    prefix = np.cumsum(onehot, axis=0)                                      # entries of the first k random points
    per_pair = np.bincount(entry_buckets(cidx)[1], minlength=nb)            # entries one (cell A, cell B) pair adds
    n_pairs = None
    for k in range(1, B // 2):
        over = (prefix[B - 2 * k] + k * per_pair).max() - cap
        if over >= 1:
            n_pairs = k
            break
    assert n_pairs is not None and over <= 8, (n_pairs, over, cap)
    x = base.copy()
    x[B - 2 * n_pairs::2] = cells[0]
    x[B - 2 * n_pairs + 1::2] = cells[1]
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(12).standard_normal((L, B, CH)) * 0.1).astype(nd)
    got = _run_bucketed(x, g, dt, times=3)
    _check_table(got, c_oracle.grid_backward(g, x, OFF, int(OFF[-1]), S, H), dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_backward_bucketed_sliced_and_spilled(dt):
    """One cell receives every 16th point of 320 K (its neighbours in the batch are random points, so nothing merges), the
    rest is uniform, and the slice length of the reduce pass is lowered to 8 K entries (lnh_grid_backward_set_slice_entries;
    default 512 K — with the dense levels' rows dealt to 64 buckets only a concentrated batch of millions of points gets
    there): every bucket of every level is reduced in slices whose images the last slice to arrive adds up; on the hashed
    levels the buckets holding that cell's corner rows receive 20 K entries on top of their even share and overflow into the
    spill list (which holds 1/16 of a level's worst case: 164 K entries), which every slice filters.  Against the oracle,
    repeated for bit equality."""
    from lidarnerf import _hip
    code = 0 if dt == torch.float32 else 1
    B = 320 * 1024
    r = np.random.default_rng(1)
    x = r.random((B, 3), dtype=np.float32)
    x[0::16] = np.float32(0.3) + r.random((B // 16, 3), dtype=np.float32) * np.float32(1e-6)
    _hip.lib().lnh_grid_backward_set_slice_entries(8192)
    try:
        nb0, cap0, _, slice_entries = _plan(B, 0, code)
        nb9, cap9, _, _ = _plan(B, 9, code)
        assert slice_entries == 8192 and B * 4 / nb0 > 2 * slice_entries and B * 4 / nb9 > 2 * slice_entries
        mean9 = B * 4 / nb9
        assert mean9 + B // 16 > cap9 + 1000                         # a hashed bucket holding one corner row overflows
        assert 4 * (mean9 + B // 16 - cap9) < B * 8 // 16            # ... and the level's spill list holds the excess
        nd = np.float32 if dt == torch.float32 else np.float16
        g = (np.random.default_rng(8).standard_normal((L, B, CH)) * 0.1).astype(nd)
        got = _run_bucketed(x, g, dt, times=2)
    finally:
        _hip.lib().lnh_grid_backward_set_slice_entries(0)
    assert _plan(B, 0, code)[3] == 512 * 1024
    want = c_oracle.grid_backward(g, x, OFF, int(OFF[-1]), S, H)
    if dt == torch.float32:
        # up to 20 K addends per row, each truncated to 2^-40 before the integer sum: one fp32 rounding on top
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    else:
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-3)
    assert np.all(got[want == 0] == 0)
    # the same batch with the default slice length (no bucket is split): bit-identical — slicing never changes a sum
    again = _run_bucketed(x, g, dt, times=1)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_backward_bucketed_smaller_workspace_means_shorter_chunks(dt):
    """Any workspace between lnh_grid_backward_workspace_size_min and lnh_grid_backward_workspace_size is accepted: the batch
    is walked in shorter chunks (one scatter + reduce pair each, the table accumulates).  Same table as the oracle; against
    the one-chunk result only the fp16 roundings move (one per row and chunk)."""
    from gpu_util import call, dev, host
    from lidarnerf import _hip
    B = 700 * 1024                                         # > 2 x 256 K points: the minimum plan walks it in 4 chunks
    x = np.concatenate([_ray_points(B // 512, 256, 21), _points(B - (B // 512) * 256, 22)])
    assert x.shape[0] == B
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(23).standard_normal((L, B, CH)) * 0.05).astype(nd)
    rows, code = int(OFF[-1]), (0 if dt == torch.float32 else 1)
    offh = torch.from_numpy(OFF)
    full = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    least = _hip.lib().lnh_grid_backward_workspace_size_min(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    assert 0 < least < 0.75 * full                         # (spill lists and slice images have floors that do not shrink)
    gd, xd = dev(g), dev(x)
    outs = {}
    for name, nbytes in (("full", full), ("least", least), ("between", (full + least) // 2)):
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
        call("lnh_grid_encode_backward_ws", gd, xd, offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, nbytes)
        outs[name] = host(ge).astype(np.float64)
        del ws
    want = c_oracle.grid_backward(g, x, OFF, rows, S, H)
    reach = c_oracle.grid_backward(np.ones((L, B, CH), dtype=np.float32), x, OFF, rows, S, H)
    for name, got in outs.items():
        _check_table(got, want, dt, untouched=(reach == 0))
    scale = np.abs(outs["full"]).max()
    assert np.abs(outs["least"] - outs["full"]).max() <= (1e-6 if dt == torch.float32 else 2e-3) * scale
    # far below the minimum (lnh_grid_backward_workspace_size_min covers every interpolation mode; this linear-interpolation
    # call gets by with somewhat less): refused, and the message names the size it needs at least
    ws = torch.empty(least // 4, dtype=torch.uint8, device="cuda")
    ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
    with pytest.raises(RuntimeError, match=r"workspace too small.*at least \d+"):
        call("lnh_grid_encode_backward_ws", gd, xd, offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, least // 4)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_backward_ws_ex_with_buffers_the_caller_cleared(dt):
    """lnh_grid_encode_backward_ws_ex: split 0 / 1 + 2 behind one signature, and the two promises a caller can make — the head
    of the workspace cleared (LNH_BWD_WS_CLEARED: the first chunk's clear launch is skipped) and the gradient table zero
    (LNH_BWD_TABLE_ZERO: the first chunk's reduce pass stores instead of read-add-store) — must give the SAME BITS as
    lnh_grid_encode_backward_ws on a garbage workspace: one chunk, several chunks (small workspace), level windows."""
    from gpu_util import call, dev
    from lidarnerf import _hip
    B = 600 * 1024
    x = np.concatenate([_ray_points(B // 512, 256, 31), _points(B - (B // 512) * 256, 32)])
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(33).standard_normal((L, B, CH)) * 0.05).astype(nd)
    rows, code = int(OFF[-1]), (0 if dt == torch.float32 else 1)
    offh = torch.from_numpy(OFF)
    full = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    least = _hip.lib().lnh_grid_backward_workspace_size_min(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    gd, xd = dev(g), dev(x)
    args = lambda ge, ws, n: (gd, xd, offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, n)
    for nbytes in (full, least):                           # one chunk / four chunks
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ws.random_(0, 255)
        ref = torch.zeros((rows, CH), dtype=dt, device="cuda")
        call("lnh_grid_encode_backward_ws", *args(ref, ws, nbytes))
        clear = _hip.lib().lnh_grid_backward_workspace_clear_bytes(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, 0, code, nbytes)
        assert 0 < clear <= 64 * 1024 and clear % 256 == 0
        for flags in (0, _hip.LNH_BWD_WS_CLEARED, _hip.LNH_BWD_TABLE_ZERO, _hip.LNH_BWD_WS_CLEARED | _hip.LNH_BWD_TABLE_ZERO):
            for windows in (None, ((0, 8), (8, 12), (12, 16))):
                ws.random_(0, 255)
                ge = torch.full((rows, CH), 9.0, dtype=dt, device="cuda")   # (cleared below by one launch, like the step does)
                _hip.zero_regions((ge, ws[:clear] if flags & _hip.LNH_BWD_WS_CLEARED else None))
                if windows is None:
                    call("lnh_grid_encode_backward_ws_ex", *args(ge, ws, nbytes), 0, L, 0, flags)
                else:
                    call("lnh_grid_encode_backward_ws_ex", *args(ge, ws, nbytes), 0, 0, 1, flags)
                    for l0, l1 in windows:
                        call("lnh_grid_encode_backward_ws_ex", *args(ge, ws, nbytes), l0, l1, 2, flags)
                assert torch.equal(ge, ref), (nbytes, flags, windows)
        del ws
    with pytest.raises(RuntimeError, match="split must be"):
        ws = torch.empty(full, dtype=torch.uint8, device="cuda")
        call("lnh_grid_encode_backward_ws_ex", *args(ref, ws, full), 0, L, 3, 0)


def test_dense_levels_are_dealt_to_64_buckets():
    """Plan of the dense plain levels (grid_pool.h bucket_of_row): rows go to min(64, ceil(rows / 128)) buckets in groups of
    128, so the few cells around the sensor that every LiDAR ray leaves are reduced by many workgroups, not one."""
    for level, rows in ((0, 17 ** 3), (1, 28 ** 3), (2, 45 ** 3), (3, 75 ** 3)):
        assert int(OFF[level + 1] - OFF[level]) >= rows
        nb = _plan(4096 * 832, level, 1)[0]
        assert nb == min(64, -(-int(OFF[level + 1] - OFF[level]) // 128)), (level, nb)
    assert _plan(4096 * 832, 4, 1)[0] == 64      # first hashed level: 2^19 rows, 8192 consecutive rows per bucket


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_backward_bucketed_spill_list_full_falls_back_to_atomics(dt):
    """HALF of 320 K points in one cell (the other half outside the grid, so no two neighbours merge): 655 K pair entries per
    level in at most 8 rows.  The hashed buckets holding those rows overflow their pools several-fold AND the level's spill
    list (164 K entries): the rest goes into the table with device atomics — the reference's own method
    (gridencoder.cu:335-350).  Still the right sums: fp32 to the accuracy of 164 K float atomics per row; fp16 tables to what
    164 K fp16 atomic adds on one row leave (the running sum outgrows the addends' precision: ~10 % — this is what the
    reference's backward does to such a batch everywhere; the bucketed path does it only past a full spill list)."""
    from gpu_util import call, dev, host
    code = 0 if dt == torch.float32 else 1
    B = 320 * 1024
    x = np.empty((B, 3), dtype=np.float32)
    x[0::2] = np.float32(0.3) + np.random.default_rng(1).random((B // 2, 3), dtype=np.float32) * np.float32(1e-6)
    x[1::2] = 1.5
    nb9, cap9, bucket_rows, _ = _plan(B, 9, code)
    # level 9: the four x-pair entries of a point go to the buckets of their even corners' rows
    rows9 = c_oracle.grid_indices(x[:1], OFF, CH, S, H)[9][0][0::2] // CH
    per_bucket = np.bincount(rows9 // bucket_rows, minlength=nb9) * (B // 2)
    assert np.maximum(per_bucket - cap9, 0).sum() > B * 8 // 16      # the excess of its buckets exceeds the level's spill list
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(8).standard_normal((L, B, CH)) * 0.1).astype(nd)
    got = _run_bucketed(x, g, dt, times=1)
    want = c_oracle.grid_backward(g, x, OFF, int(OFF[-1]), S, H)
    assert np.isfinite(got).all() and np.all(got[want == 0] == 0)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert rel < (1e-4 if dt == torch.float32 else 0.25), rel
    # The same batch through lnh_grid_encode_backward_ws_ex with the promises of the training step (workspace head cleared,
    # gradient table zero: the reduce pass would STORE its sums over the rows): the entries the scatter pass added with
    # atomics must survive — on such a level the reduce pass reads the rows whatever the flag says.  (Rounds 5: they were
    # overwritten; found by review, never by a test: this combination was not covered.)
    from lidarnerf import _hip
    offh, rows = torch.from_numpy(OFF), int(OFF[-1])
    need = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    clear = _hip.lib().lnh_grid_backward_workspace_clear_bytes(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, 0, code, need)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    gd, xd = dev(g), dev(x)
    for flags in (_hip.LNH_BWD_TABLE_ZERO, _hip.LNH_BWD_WS_CLEARED | _hip.LNH_BWD_TABLE_ZERO):
        ws.random_(0, 255)
        ge = torch.full((rows, CH), 9.0, dtype=dt, device="cuda")
        _hip.zero_regions((ge, ws[:clear] if flags & _hip.LNH_BWD_WS_CLEARED else None))
        call("lnh_grid_encode_backward_ws_ex", gd, xd, offh, ge, B, 3, CH, L, S, H, 0, 0, 0, code, ws, need, 0, L, 0, flags)
        got_f = host(ge).astype(np.float64)
        assert np.isfinite(got_f).all() and np.all(got_f[want == 0] == 0)
        rel_f = np.linalg.norm(got_f - want) / np.linalg.norm(want)
        assert rel_f < (1e-4 if dt == torch.float32 else 0.25), (flags, rel_f)
    # rows no point of the batch touches stay exactly zero; every other level's hot rows went the same way (level 0 too: its
    # rows are dealt to 38 buckets, the four holding the cell's even corners overflow like the hashed ones)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("interp,gridtype,align", [(1, 0, False), (0, 1, False), (0, 0, True)])
def test_backward_bucketed_generic_level_classes(dt, interp, gridtype, align):
    """Smoothstep interpolation, tiled grids and align_corners take the generic class of the bucketed backward: every
    corner travels as a single entry (8 per point, more than the workgroup's LDS staging holds — the excess is written
    straight to its slot).  Same table as the oracle, ray-ordered points (run-merge active) and random ones."""
    from gpu_util import call, dev, host
    from lidarnerf import _hip
    off = grid_ref.make_offsets(3, L, PLS, H, 19, align_corners=align)
    x = np.concatenate([_ray_points(24, 256, 13), _points(3000, 14)])
    B, rows = x.shape[0], int(off[-1])
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(15).standard_normal((L, B, CH)) * 0.1).astype(nd)
    # zero-gradient samples among the ray-ordered points: sprinkled ones (silent members of their runs) and the far end of
    # every ray (dropped before the pool)
    zr = np.random.default_rng(16).random(24 * 256) < 0.4
    zr.reshape(24, 256)[:, 200:] = True
    g[:, :24 * 256][:, zr] = 0
    want = c_oracle.grid_backward(g, x, off, rows, S, H, gridtype, align, interp)
    code = 0 if dt == torch.float32 else 1
    offh = torch.from_numpy(off)
    need = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, gridtype, int(align), code)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
        call("lnh_grid_encode_backward_ws", dev(g), dev(x), offh, ge, B, 3, CH, L, S, H, gridtype, int(align), interp,
             code, ws, need)
        outs.append(ge)
    assert torch.equal(outs[0], outs[1])
    _check_table(host(outs[0]).astype(np.float64), want, dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
def test_backward_bucketed_generic_class_overflow(dt):
    """The generic scatter kernel's spill branch: a bucket of a generic-class level outgrows its pool share.  Smoothstep
    interpolation makes every level generic (8 singles per point).  B = 8192: a hashed level has a worst case of 65536
    entries over 64 buckets, so its pool share (plan_buckets) is 1024 + 1024 / 8 + 12 * sqrt(1024) + 64 = 1600 slots per
    bucket.  Points 0..4095 alternate between two cells (alternating, so the run-merge cannot collapse them): every corner
    row of either cell receives 2048 entries, so at least one bucket overflows whatever the hash does.  The spill list holds
    the level's whole worst case at this size (min(max(65536 / 16, 2^20), 65536)), so no float atomic is reached and the
    sum is exact: equal to the oracle, and bit-identical run to run."""
    from gpu_util import call, dev, host
    from lidarnerf import _hip
    B, rows = 8192, int(OFF[-1])
    x = np.random.default_rng(21).random((B, 3), dtype=np.float32)
    x[0:4096:2] = 0.3
    x[1:4096:2] = 0.41
    nd = np.float32 if dt == torch.float32 else np.float16
    g = (np.random.default_rng(22).standard_normal((L, B, CH)) * 0.1).astype(nd)
    want = c_oracle.grid_backward(g, x, OFF, rows, S, H, 0, False, 1)
    code = 0 if dt == torch.float32 else 1
    offh = torch.from_numpy(OFF)
    need = _hip.lib().lnh_grid_backward_workspace_size(offh.data_ptr(), B, 3, CH, L, S, H, 0, 0, code)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    gd, xd = dev(g), dev(x)
    outs = []
    for _ in range(2):
        ge = torch.zeros((rows, CH), dtype=dt, device="cuda")
        call("lnh_grid_encode_backward_ws", gd, xd, offh, ge, B, 3, CH, L, S, H, 0, 0, 1, code, ws, need)
        outs.append(ge)
    assert torch.equal(outs[0], outs[1])
    _check_table(host(outs[0]).astype(np.float64), want, dt)


def test_error_paths():
    from lidarnerf import _hip
    x = torch.rand((8, 3), device="cuda")
    out = torch.empty((L, 8, 3), device="cuda")
    emb = torch.zeros((int(OFF[-1]), 3), device="cuda")
    with pytest.raises(RuntimeError, match="C must be 1, 2, 4, or 8"):
        _hip.call("lnh_grid_encode_forward", x.data_ptr(), emb.data_ptr(), torch.from_numpy(OFF).data_ptr(),
                  out.data_ptr(), 8, 3, 3, L, S, H, None, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="D must be"):
        _hip.call("lnh_grid_encode_forward", x.data_ptr(), emb.data_ptr(), torch.from_numpy(OFF).data_ptr(),
                  out.data_ptr(), 8, 7, 2, L, S, H, None, 0, 0, 0, 0)
    # empty batch is a no-op
    _hip.call("lnh_grid_encode_forward", x.data_ptr(), emb.data_ptr(), torch.from_numpy(OFF).data_ptr(),
              out.data_ptr(), 0, 3, 2, L, S, H, None, 0, 0, 0, 0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("gridtype,align", [(0, False), (1, False), (0, True)])
def test_grad_total_variation(dt, gridtype, align):
    """lnh_grad_total_variation vs the C restatement of kernel_grad_tv (gridencoder.cu:695-807): the increment added to
    an existing gradient.  fp32: float atomics (order) and the hardware rsqrt; fp16: the kernel's locals are __half in the
    reference (every difference, running sum and square rounded), accumulated with fp16 atomics."""
    from gpu_util import call, dev, host
    x = _points(3000, 21)
    off = grid_ref.make_offsets(3, L, PLS, H, 19, align_corners=align)
    r = np.random.default_rng(22)
    npdt = np.float32 if dt == torch.float32 else np.float16
    emb = r.standard_normal((int(off[-1]), CH)).astype(npdt)
    g0 = (r.standard_normal((int(off[-1]), CH)) * 1e-3).astype(npdt)
    xin = x.astype(npdt)  # the entry point reads `inputs` in the table type, as the reference's kernel does
    want = c_oracle.grad_total_variation(xin.astype(np.float32), emb, off, 1e-2, S, H, gridtype, align)
    grad = dev(g0.copy())
    call("lnh_grad_total_variation", dev(xin), dev(emb), grad, torch.from_numpy(off), 1e-2, x.shape[0], 3, CH, L, S, H,
         gridtype, int(align), 0 if dt == torch.float32 else 1)
    got = host(grad).astype(np.float64) - g0.astype(np.float64)
    touched = want != 0
    assert touched.sum() > 1000
    if dt == torch.float32:
        np.testing.assert_allclose(got, want, rtol=0, atol=3e-6 * np.abs(want).max())
    else:
        # rows hit by many points (coarse levels) accumulate fp16 roundings of a running sum: compare in norm and loosely
        # per entry; untouched rows must stay bit-identical
        assert np.linalg.norm(got - want) <= 3e-3 * np.linalg.norm(want)
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-2 * np.abs(want).max())
    assert np.all(got[~touched] == 0)


def test_grad_total_variation_module_matches_entry_point():
    """GridEncoder.grad_total_variation (grid.py:237-277 API): adds into embeddings.grad, bound mapping included."""
    from lidarnerf.gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=8, level_dim=2, base_resolution=16, log2_hashmap_size=15,
                      desired_resolution=512).cuda()
    with torch.no_grad():
        enc.embeddings.uniform_(-1, 1)
    enc.embeddings.grad = torch.zeros_like(enc.embeddings)
    pts = (torch.rand(500, 3, device="cuda") * 2 - 1) * 2.0  # bound = 2
    enc.grad_total_variation(weight=1e-3, inputs=pts, bound=2)
    off = enc.offsets.cpu().numpy()
    x01 = ((pts + 2) / 4).cpu().numpy()
    want = c_oracle.grad_total_variation(x01, enc.embeddings.detach().cpu().numpy(), off, 1e-3, enc.log2_scale,
                                         enc.base_resolution)
    np.testing.assert_allclose(enc.embeddings.grad.cpu().numpy(), want, rtol=0, atol=3e-6 * np.abs(want).max())
