"""The exact known-answer cases of the hash-grid table backward (tests/grid_exact_cases.py), checked without a GPU: the
conditions that make the integer table the one right answer in any summation order, integer reference == C oracle ==
NumPy oracle bit for bit, presence of every structural class the GPU test relies on (computed from the data: point index
mod 64 and mod 1024, cell ids per level, row codes), and sensitivity — each classic mistake applied to the REFERENCE
changes the expected table of the case meant to catch it."""
import numpy as np
import pytest

import grid_exact_cases as X
from oracle import c_oracle, grid_ref

L = X.L
_CACHE = {}


def _case(name, f16):
    key = (name, f16)
    if key not in _CACHE:
        if name in ("smoothstep", "tiled", "align"):
            c = X.case_generic(f16, name)
        elif name.startswith("atomic"):
            _, D, C = name.split("_")
            c = X.case_atomic(f16, int(D), int(C))
        elif name == "hot_cell":
            c = X.case_hot_cell(f16, 4096, 1024)
        elif name == "chunked":
            c = X.case_chunked(f16, 256 * 1024 + 1)
        elif name == "window":
            b = X.case_runs_small(f16)
            c = X.Case("window", f16, b.M, b.k, b.gn, b.q, window=(8, 12))
        else:
            c = getattr(X, "case_" + name)(f16)
        _CACHE[key] = (c, c.check_conditions())
    return _CACHE[key]


CASES = ["runs", "runs_small", "min_merges", "zeros", "pairs", "tcnn", "smoothstep", "tiled", "align", "hot_cell", "window",
         "unstaged", "chunked"]
ATOMIC = [f"atomic_{D}_{C}" for D in (2, 3, 4) for C in (1, 2, 4, 8)]


# (fp16 tables have an even number of channels — the reference forces fp32 for odd C — so C = 1 is an fp32 case only)
@pytest.mark.parametrize("name,f16", [(n, f) for n in CASES + ATOMIC for f in (False, True) if not (f and n in ATOMIC and n.endswith("_1"))],
                         ids=lambda v: v if isinstance(v, str) else ("f16" if v else "f32"))
def test_conditions_and_oracles(name, f16):
    """check_conditions (C1, the fp32 cap, the fp16 caps a / b / c) and reference == c_oracle == grid_ref, bit for bit."""
    c, tab = _case(name, f16)
    want = c.exact(tab)
    assert np.any(tab != 0)
    if name.startswith("atomic") and f16:
        assert X.atomic_fp16_row_cap(c)
    if c.window != (0, L) or c.gridtype == 2:
        return  # (the oracles have no level window and no tiny-cuda-nn lattice)
    g = c.grad()
    got = c_oracle.grid_backward(g, c.x, c.off, c.rows_total, X.S, X.H, c.gridtype, c.align, c.interp)
    np.testing.assert_array_equal(got, want)
    if name == "unstaged":   # all_staged == false and pad_unstaged of the plain scatter kernel
        assert X.unstaged_facts(c, 9) == (True, True) and X.unstaged_facts(c, 0) == (False, False)
    if name == "chunked":
        assert X.atomic_fp16_row_cap(c)
    if c.B <= 8192 and c.C <= 2:
        np.testing.assert_array_equal(grid_ref.backward(g, c.x, c.off, c.rows_total, X.S, X.H, c.gridtype, c.align, c.interp), want)
    if f16 and name == "runs":
        # the final rounding is exercised: some row totals are not fp16 numbers
        assert np.any(c.to_table(tab).astype(np.float64) != want)


def test_tcnn_rows_match_the_restatement_of_the_geometry_tests():
    """gridtype 2 rows: same levels and offsets as lidarnerf's level_offsets would give is pinned on the GPU
    (test_grid_exact_gpu.py compares lnh_grid_corner_indices with Case.rows); here: dense levels 0..2 with stride res."""
    lv = X.tcnn_levels(3)
    assert [h for _, _, h in lv] == [False] * 3 + [True] * 9 + [False] * 4    # (levels 12..15: the uint32 stride wraps)
    assert [r for r, _, _ in lv[:3]] == [16, 32, 64] and [n for _, n, _ in lv[:3]] == [16 ** 3, 32 ** 3, 64 ** 3]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_coverage_run_classes(f16):
    """1. every required run length starting at every lane; runs crossing 15|16, 31|32, 47|48, the wave boundary and the
    workgroup boundary; on every level (the runs are repeated lattice points).  fp32: a run on level 0 that is none on 1."""
    c, _ = _case("runs", f16)
    for level in (0, 2, 3, 15):
        st, ln = X.batch_runs(c, level)
        have = set(zip(ln.tolist(), (st % 64).tolist()))
        for n in X.RUN_LENGTHS[:-1]:
            assert all((n, s) in have for s in range(64)), (level, n)
        long_starts = {s % 64 for s, n in zip(st.tolist(), ln.tolist()) if n >= 130}
        assert long_starts == set(range(64)), level
        inside = np.zeros(c.B + 1, dtype=bool)     # index i: points i - 1 and i belong to one run
        for s, n in zip(st.tolist(), ln.tolist()):
            inside[s + 1:s + n] = True
        idx = np.flatnonzero(inside)
        for lane in (16, 32, 48, 0):
            assert np.any(idx % 64 == lane), (level, lane)
        assert np.any(idx % 1024 == 0), level
        # the scan steps: dense levels continue across the 16-lane rows, hashed ones do not
        _, cont = X.emits(c, level)
        lane = np.arange(c.B) % 64
        assert np.any(cont & (lane == 32)) == (not c.hashed(level)) and np.any(cont & (lane == 16)) == (not c.hashed(level))
        assert not np.any(cont & (lane == 0))
    if not f16:
        n0, n1 = X.batch_runs(c, 0)[1], X.batch_runs(c, 1)[1]
        tail = slice(c.B - 256, c.B)
        r0, r1 = c.run_ids(0)[0][tail], c.run_ids(1)[0][tail]
        # the 1/32-lattice neighbours: ONE run of 256 on level 0, 256 runs of one on level 1
        assert len(set(r0.tolist())) == 1 and len(set(r1.tolist())) == 256 and n0.max() >= 256 and 130 <= n1.max() < 256


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_coverage_min_merges(f16):
    c, _ = _case("min_merges", f16)
    for level in (0, 5):
        member, nz, cont = X.structure(c, level)
        per_wave = cont.reshape(-1, 64).sum(axis=1).tolist()
        assert per_wave == [0, 1, 7, 8, 9], (level, per_wave)
        _, kept = X.emits(c, level)
        assert kept.reshape(-1, 64).sum(axis=1).tolist() == [0, 0, 0, 8, 9]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_coverage_zeros(f16):
    c, _ = _case("zeros", f16)
    g = c.grad()
    level = 2
    zero = ~np.any(c.gn[level] != 0, axis=1)
    member, nz, cont = X.structure(c, level)
    kinds = {m[2] for m in c.marks}
    assert kinds == {"inner", "head", "tail", "all_zero", "neg_zero", "one_channel", "one_level", "bad_hi", "bad_lo"}
    for s, n, what, *a in c.marks:
        sl = slice(s, s + n)
        if what == "inner":
            z = a[1]
            assert zero[sl].sum() == z
            # six are bridged from both ends (every zero is a member), seven leave a non-member: the run is cut
            assert member[sl].all() == (z <= 6)
        elif what == "tail":
            assert zero[s + n - 1] and not zero[s]
        elif what == "head":
            assert zero[s] and not zero[s + n - 1]
        elif what == "all_zero":
            assert zero[sl].all()       # (zeros within three lanes of a neighbouring run's gradient are silent members)
            assert not (member[sl].any() if n == 64 else member[s + 3:s + n - 3].any())
        elif what == "neg_zero":
            assert np.signbit(g[level, s + 2]).all() and (g[level, s + 2] == 0).all()
            assert np.signbit(g[level, s + 7, 1]) and g[level, s + 7, 0] != 0
        elif what == "one_channel":
            assert (c.gn[level, s + 3:s + 9, 0] == 0).all() and (c.gn[level, s + 3:s + 9, 1] != 0).all()
        elif what == "one_level":
            assert (c.gn[1, s + 4] == 0).all() and (c.gn[2, s + 4] != 0).all()
        else:
            p = s + a[0]
            assert not c.valid[p] and c.valid[p - 1] and c.valid[p + 1]
            assert np.all(c.M[p - 1] == c.M[p + 1])            # it sits inside a run and cuts it
    assert any(n == 64 and s % 64 == 0 for s, n, what, *a in c.marks if what == "all_zero")
    assert (c.x == 0).all(axis=1).any() or (c.x == 0).any()
    assert (c.x == 1).any() and (c.x == 0).any()
    assert np.float32(1.0000001) > 1 and np.float32(-1e-7) < 0


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_coverage_pairs_and_singles(f16):
    """4. hashed levels: every pair code 0..6 and the single code 7; dense levels: pairs with r0 & 127 == 127 beside ordinary
    ones; a workgroup with an odd entry count for a bucket (the zero padding entry)."""
    c, _ = _case("pairs", f16)
    codes = set()
    for level in range(3, L):
        assert c.hashed(level)
        nz = np.any(c.gn[level] != 0, axis=1)
        codes |= set(c.pair_codes(level)[nz].ravel().tolist())
    assert codes == set(range(8)), codes
    dense = set()
    for level in range(3):
        assert not c.hashed(level)
        dense |= set(c.pair_codes(level).ravel().tolist())
    assert dense == {0, 7}
    odd = False
    for level in range(L):
        wg, bk = X.plain_entry_buckets(c, level)
        odd |= bool(np.any(np.bincount(wg * 64 + bk) % 2 == 1))
    assert odd


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_coverage_tcnn_and_generic(f16):
    c, _ = _case("tcnn", f16)
    for level in range(3):       # the pair whose first row is the level's last row: wraps to row 0, two singles
        rows = c.rows(level)
        last = int(c.off[level + 1] - c.off[level]) - 1
        assert np.any((rows[:, 0::2] == last) & (rows[:, 1::2] == 0)), level
    for name in ("smoothstep", "tiled", "align"):
        g, _ = _case(name, f16)
        assert g.B > 2 * 1024
        # a whole workgroup in which nobody merges: 8 * 1024 singles, more than the 6144 staging slots
        for level in (0, 9):
            emit, cont = X.emits(g, level)
            per_wg = emit[:g.B // 1024 * 1024].reshape(-1, 1024).sum(axis=1)
            assert np.any(per_wg * 8 > 6144), (name, level)
        _, cont = X.emits(g, 0)
        assert cont.any() and (~g.valid).any() and np.any(~np.any(g.gn[0] != 0, axis=1))


SENSITIVE = {
    "run_last_dropped": "runs", "run_across_cell_change": "runs", "pair_row_plus1_on_hashed": "pairs",
    "pair_row_xor_on_dense": "pairs", "straddling_second_corner_dropped": "pairs", "zero_tail_run_not_emitted": "zeros",
    "out_of_range_contributes": "zeros", "overflow_entry_lost": "hot_cell", "slice_image_not_added": "hot_cell",
    "level_outside_window_written": "window",
}


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("mistake", X.MUTATIONS)
def test_sensitivity(mistake, f16):
    """The expected TABLE (after the rounding to the table type) of the case meant to catch a mistake differs from the table
    the mistake produces."""
    c, tab = _case(SENSITIVE[mistake], f16)
    wrong = c.reference(mutate=mistake)
    a, b = c.to_table(tab), c.to_table(wrong)
    assert not np.array_equal(a, b), mistake
    assert set(SENSITIVE) == set(X.MUTATIONS)
