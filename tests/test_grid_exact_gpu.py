"""Exact known-answer tests of the hash-grid table backward on the GPU: lnh_grid_encode_backward_ws and its entry points
(grid_bwd_scatter.hip, grid_bwd_reduce.hip, grid_pool.h) and the atomic lnh_grid_encode_backward, against the integer
reference of tests/grid_exact_cases.py with torch.equal — fp32 and fp16 tables.  The inputs sit on a dyadic lattice on
which every contribution and every sum is an integer number of units, so the table has ONE right value whatever the order
of summation (the conditions are asserted by Case.check_conditions; tests/test_grid_exact_cpu.py checks them, the
presence of every structural class and the sensitivity of every case without a GPU).  Every call runs twice on a
workspace filled with random bytes, into a table with guard words behind it."""
import numpy as np
import pytest
import torch

import grid_exact_cases as X
from exact_util import Out, _twice

pytestmark = pytest.mark.gpu

L, CH, S, H = X.L, X.CH, X.S, X.H
DT = pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
WINDOWS = ((0, 8), (8, 12), (12, 16))


class Dev:
    """Device side of a case."""

    def __init__(self, c):
        from gpu_util import dev
        self.c = c
        self.dt = torch.float16 if c.f16 else torch.float32
        self.code = 1 if c.f16 else 0
        self.x, self.g = dev(c.x), dev(c.grad())
        self.offh = torch.from_numpy(c.off)

    def size(self, fn="lnh_grid_backward_workspace_size"):
        from lidarnerf import _hip
        c = self.c
        n = getattr(_hip.lib(), fn)(self.offh.data_ptr(), c.B, 3, CH, L, S, H, c.gridtype, int(c.align), self.code)
        assert n > 0
        return n

    def args(self, table, ws, nbytes):
        c = self.c
        return (self.g, self.x, self.offh, table, c.B, 3, CH, L, S, H, c.gridtype, int(c.align), c.interp, self.code, ws, nbytes)


def _want(c, units):
    return torch.from_numpy(c.to_table(units)).cuda()


def _run(d, want, what, steps=None, nbytes=None, prefill=None, cleared=False):
    """`steps`: the calls of one backward, (entry point, extra arguments) each; default: lnh_grid_encode_backward_ws.
    cleared: the caller clears the head of the workspace itself (LNH_BWD_WS_CLEARED)."""
    from gpu_util import call
    from lidarnerf import _hip
    c = d.c
    nbytes = nbytes or d.size()
    steps = steps or (("lnh_grid_encode_backward_ws", ()),)

    def once():
        out = Out((c.rows_total, CH), d.dt, fill=0.0)
        if prefill is not None:
            out.data().copy_(prefill)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ws.random_(0, 255)
        if cleared:
            clear = _hip.lib().lnh_grid_backward_workspace_clear_bytes(d.offh.data_ptr(), c.B, 3, CH, L, S, H, c.gridtype,
                                                                       int(c.align), c.interp, d.code, nbytes)
            assert 0 < clear <= 64 * 1024
            _hip.zero_regions((ws[:clear],))
        for entry, extra in steps:
            call(entry, *d.args(out.data(), ws, nbytes), *extra)
        torch.cuda.synchronize()
        return (out,)

    (out,) = _twice(once)
    out.check(want, f"{c.name} {what}")
    return out


# ---- 1-5: the plain scatter kernel's structural classes
@DT
@pytest.mark.parametrize("name", ["runs", "min_merges", "zeros", "pairs", "unstaged", "tcnn"])
def test_plain_classes(name, f16):
    c = getattr(X, "case_" + name)(f16)
    tab = c.check_conditions()
    if name == "unstaged":
        assert X.unstaged_facts(c, 9) == (True, True)      # all_staged == false, and a padding entry beyond the staging area
    if name == "tcnn":   # the rows of the restatement are the kernel's
        from gpu_util import call, dev, host
        from lidarnerf.gridencoder import grid
        assert np.array_equal(grid.level_offsets(3, L, 2.0, H, X.LOG2, False, gridtype="tcnn"), c.off)
        idx = torch.empty((L, c.B, 8), dtype=torch.int32, device="cuda")
        call("lnh_grid_corner_indices", dev(c.x), torch.from_numpy(c.off), idx, c.B, 3, CH, L, S, H, 2, 0)
        got = host(idx).view(np.uint32).astype(np.int64) // CH
        for level in range(L):
            assert np.array_equal(got[level], c.rows(level)), level
    _run(Dev(c), _want(c, tab), "ws")


# ---- 6: the generic classes (k_grid_bwd_scatter: its own scan, eight singles per point, the staging bypass)
@DT
@pytest.mark.parametrize("which", ["smoothstep", "tiled", "align"])
def test_generic_classes(which, f16):
    c = X.case_generic(f16, which)
    tab = c.check_conditions()
    emit, _ = X.emits(c, 9)
    assert np.any(emit[:c.B // 1024 * 1024].reshape(-1, 1024).sum(axis=1) * 8 > 6144)
    _run(Dev(c), _want(c, tab), "ws")


# ---- 7: pool overflow
def _plan(c, level, code):
    from lidarnerf import _hip
    out = np.zeros(4, dtype=np.uint32)
    rc = _hip.lib().lnh_grid_backward_plan_info(torch.from_numpy(c.off).data_ptr(), c.B, 3, CH, L, S, H, c.gridtype,
                                                int(c.align), code, level, out.ctypes.data)
    assert rc == 0
    return [int(v) for v in out]


@DT
@pytest.mark.parametrize("cls", ["plain", "generic"])
def test_pool_overflow_by_a_few(cls, f16):
    """The fullest bucket of one hashed level reserves 1..8 slots more than its pool holds: they take the spill list."""
    kw = dict(align=True) if cls == "generic" else {}
    B = 8192 if cls == "generic" else 12288
    probe = X.case_hot_cell(f16, B, 0, **kw)
    caps = {level: _plan(probe, level, int(f16))[1] for level in range(3, L)}
    c, level, over = X.case_overflow_by_a_few(f16, B, caps.get, plain=(cls == "plain"), **kw)
    assert 1 <= over <= 8 and _plan(c, level, int(f16))[0] == 64, (level, over)
    _run(Dev(c), _want(c, c.check_conditions()), f"overflow by {over} on level {level}")


@DT
def test_spill_entries_filtered_by_several_slices(f16):
    """Half the batch alternates between two cells, the reduce slice is cut to 1024 entries: every bucket is reduced in
    several slices, the buckets of the two cells overflow into the spill list, which every slice filters."""
    from lidarnerf import _hip
    c = X.case_hot_cell(f16, 32768, 16384, k=4, x_coarse=True)
    want = _want(c, c.check_conditions())
    d = Dev(c)
    _hip.lib().lnh_grid_backward_set_slice_entries(1024)
    try:
        nb, cap, _, per_slice = _plan(c, 9, d.code)
        slots = X.reserved_slots(c, 9)[0]
        assert per_slice == 1024 and slots.max() > cap + 1000 and slots.max() > 4 * per_slice and np.median(slots) > per_slice
        _run(d, want, "sliced")
    finally:
        _hip.lib().lnh_grid_backward_set_slice_entries(0)
    assert _plan(c, 9, d.code)[3] == 512 * 1024
    _run(d, want, "unsliced")


# ---- 8: spill list full -> device atomics (fp32: the sum is exact, hence order-free)
def test_spill_list_full_falls_back_to_atomics_exactly():
    from lidarnerf import _hip
    c = X.case_spill_full()
    want = _want(c, c.check_conditions())
    d = Dev(c)
    # the level's spill list holds max(B * 8 / 16, 2^20) entries (plan_buckets, grid_bwd_reduce.hip); what the buckets of
    # level 9 reserve beyond their pools exceeds it
    nb, cap, _, _ = _plan(c, 9, 0)
    slots = X.reserved_slots(c, 9)[0]
    spill_cap = min(max(c.B * 8 // 16, 1 << 20), c.B * 8)
    assert np.maximum(slots - cap, 0).sum() > spill_cap, (np.maximum(slots - cap, 0).sum(), spill_cap)
    _run(d, want, "ws")
    for flags in (_hip.LNH_BWD_TABLE_ZERO, _hip.LNH_BWD_WS_CLEARED | _hip.LNH_BWD_TABLE_ZERO):
        _run(d, want, f"ws_ex flags {flags}", steps=(("lnh_grid_encode_backward_ws_ex", (0, L, 0, flags)),),
             cleared=bool(flags & _hip.LNH_BWD_WS_CLEARED))


# ---- 9: entry points and table state
@DT
def test_entry_points_and_table_state(f16):
    from lidarnerf import _hip
    c = X.case_runs_small(f16)
    tab = c.check_conditions()
    d = Dev(c)
    want = _want(c, tab)
    for flags in (0, _hip.LNH_BWD_WS_CLEARED, _hip.LNH_BWD_TABLE_ZERO, _hip.LNH_BWD_WS_CLEARED | _hip.LNH_BWD_TABLE_ZERO):
        cleared = bool(flags & _hip.LNH_BWD_WS_CLEARED)
        _run(d, want, f"ws_ex split 0 flags {flags}", steps=(("lnh_grid_encode_backward_ws_ex", (0, L, 0, flags)),), cleared=cleared)
        steps = (("lnh_grid_encode_backward_ws_ex", (0, 0, 1, flags)),) + tuple(
            ("lnh_grid_encode_backward_ws_ex", (l0, l1, 2, flags)) for l0, l1 in WINDOWS)
        _run(d, want, f"ws_ex split 1 + 2 flags {flags}", steps=steps, cleared=cleared)
    # a table that is NOT zero on entry: prefill + sum, and rows of levels outside the window bit-unchanged.  The prefill is a
    # multiple of 8 units below 2^6: prefill + sum keeps 24 significant bits, the one rounding is the table type's
    pre_units = np.random.default_rng(9).integers(-4, 5, (c.rows_total, CH)) * 8
    pre = _want(c, pre_units)
    assert torch.equal(pre.double(), torch.from_numpy(c.exact(pre_units)).cuda())
    _run(d, _want(c, pre_units + tab), "ws on a prefilled table", prefill=pre)
    steps = (("lnh_grid_encode_backward_ws_begin", ()),) + tuple(("lnh_grid_encode_backward_ws_finish", w) for w in WINDOWS)
    _run(d, _want(c, pre_units + tab), "begin + finish on a prefilled table", steps=steps, prefill=pre)
    win = X.Case("window", f16, c.M, c.k, c.gn, c.q, window=(8, 12))
    win.x, win.valid = c.x, c.valid
    wtab = win.check_conditions()
    assert np.all(wtab[:c.off[8]] == 0) and np.all(wtab[c.off[12]:] == 0) and np.any(wtab != 0)
    _run(d, _want(c, pre_units + wtab), "ws_levels (8, 12) on a prefilled table",
         steps=(("lnh_grid_encode_backward_ws_levels", (8, 12)),), prefill=pre)


# ---- 10: chunked batch
@DT
def test_chunked_batch_in_the_minimum_workspace(f16):
    from lidarnerf import _hip
    B = 256 * 1024 + 1
    off = torch.from_numpy(X.offsets())
    sizes = lambda b: [getattr(_hip.lib(), "lnh_grid_backward_workspace_size" + sfx)(off.data_ptr(), b, 3, CH, L, S, H, 0, 0, int(f16))
                       for sfx in ("", "_min")]
    full, least = sizes(B)
    assert least < full and sizes(B - 1)[0] == sizes(B - 1)[1]    # the smallest batch the minimum plan cuts in two
    c = X.case_chunked(f16, B)
    tab = c.check_conditions()
    assert X.atomic_fp16_row_cap(c)     # per row the sum of |units| over all chunks keeps 11 bits: no chunk's rounding bites
    live = np.flatnonzero(np.any(c.gn[0] != 0, axis=1))
    assert live[0] == 0 and live[-1] == B - 1 and np.any((live > 1024) & (live < B // 2)) and np.any(live > B // 2 + 1024)
    d = Dev(c)
    _run(d, _want(c, tab), "minimum workspace", nbytes=least)
    _run(d, _want(c, tab), "full workspace", nbytes=full)


# ---- 11: the atomic entry point
@DT
@pytest.mark.parametrize("C", [1, 2, 4, 8])
@pytest.mark.parametrize("D", [2, 3, 4])
def test_atomic_entry_point(D, C, f16):
    from gpu_util import call
    c = X.case_atomic(f16, D, C)
    d_off = torch.from_numpy(c.off)
    from gpu_util import dev
    x, g = dev(c.x), dev(c.grad())
    if f16 and C == 1:
        out = Out((c.rows_total, C), torch.float16, fill=0.0)
        with pytest.raises(RuntimeError, match="even C"):
            call("lnh_grid_encode_backward", g, x, None, d_off, out.data(), c.B, D, C, L, S, H, None, None, 0, 0, 0, 1)
        return
    tab = c.check_conditions()
    if f16:
        assert X.atomic_fp16_row_cap(c)

    def once():
        out = Out((c.rows_total, C), torch.float16 if f16 else torch.float32, fill=0.0)
        call("lnh_grid_encode_backward", g, x, None, d_off, out.data(), c.B, D, C, L, S, H, None, None, 0, 0, 0, int(f16))
        torch.cuda.synchronize()
        return (out,)

    (out,) = _twice(once)
    out.check(_want(c, tab), c.name)


# ---- overflowed gradients, fp16 tables.  (fp32 training runs without a loss scaler, and the fp32 conversion of the reduce
# pass, (long long)ldexp(inf, 40), is undefined anyway: nothing to pin there.)
def _nonfinite_case(place):
    if place == "no_scan":        # wave 0 of the kMinMerges case: no continuing lane
        c = X.case_min_merges(True)
        return c, 5
    if place == "merged_run":     # its last wave: a run of ten at the wave's start, scanned
        c = X.case_min_merges(True)
        return c, 4 * 64 + 3
    c = X.case_hot_cell(True, 8192, 4096, k=4, x_coarse=True)   # the hot buckets overflow from the second workgroup on
    return c, 4094


@pytest.mark.parametrize("place", ["no_scan", "merged_run", "spilling_bucket"])
@pytest.mark.parametrize("value", ["inf", "-inf", "nan"])
def test_nonfinite_gradient_reaches_the_table(value, place):
    """lnh_train_check looks for inf / NaN in the fp16 table gradient: a non-finite upstream gradient of one in-range sample
    must leave a non-finite value in at least one of the sample's corner rows (non-zero weight) on every level of the window,
    and rows of levels outside the window stay finite."""
    from gpu_util import call, host
    c, p = _nonfinite_case(place)
    assert c.valid[p]
    d = Dev(c)
    g = c.grad()
    g[:, p, 0] = np.float16(value)
    d.g = torch.from_numpy(g).cuda()
    l0, l1 = 2, 11
    nbytes = d.size()
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ws.random_(0, 255)
    out = Out((c.rows_total, CH), torch.float16, fill=0.0)
    call("lnh_grid_encode_backward_ws_levels", *d.args(out.data(), ws, nbytes), l0, l1)
    got = host(out.data()).astype(np.float32)
    assert np.isfinite(got[:c.off[l0]]).all() and np.isfinite(got[c.off[l1]:]).all()
    for level in range(l0, l1):
        rows = c.rows(level)[p] + int(c.off[level])
        w = c.weights(level, np.array([p]))[0]
        assert (w != 0).any()
        assert not np.isfinite(got[rows[w != 0], 0]).all(), (level, got[rows[w != 0], 0])
