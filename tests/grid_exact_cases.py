"""Exact known-answer cases for the hash-grid table backward (tests/test_grid_exact_cpu.py, tests/test_grid_exact_gpu.py).

The construction: per-level scale 2 (S = 1), H = 16, L = 16, 2^19 rows — the level scale is 16 * 2^l - 1 exactly.  Every
coordinate is x = m / 2^k, so pos = x * scale + 0.5 = (m * scale + 2^(k-1)) / 2^k is a dyadic number the float32 fma holds
exactly (k <= 5: 19 integer bits + k <= 24), the trilinear weights are integer multiples of 2^-3k (smoothstep: 2^-9k), and
with gradients n * 2^-q every contribution and every sum is an integer number of UNITS 2^-(3k + q).  The right table is
integer arithmetic: `Case.reference()` below, int64 from the lattice to the last add.  It takes the corner rows from the C
oracle's index function (gridtypes 0 and 1) or from tiny-cuda-nn's published index rule (gridtype 2) and knows nothing
about waves, pools or buckets.  What makes that table the ONE right answer in any summation order are properties of the
inputs, checked by `Case.check_conditions()`:
  C1    pos is exactly representable in float32 for every (point, level) that carries a gradient;
  fp32  per row and channel the sum of |contributions| has at most 24 significant bits above their common unit: every
        partial sum — run-merge order, pool order, float-atomic arrival order — is exact;
  fp16  (a) every contribution has at most 11 significant bits (the per-contribution rounding is the identity);
        (b) over every maximal stretch of consecutive batch indices in one cell of a level, per corner and channel, the sum
            of |contributions| has at most 11 significant bits above their common unit: whatever contiguous piece a scan
            merges, its fp32 sum rounds to fp16 unchanged;
        (c) every row total has at most 24 significant bits: the reduce pass's float step is exact, the one remaining
            rounding is round-to-nearest-even — expected = float16(exact).
("n significant bits above the common unit": sum < 2^n * u, u the largest power of two dividing every addend.  Where the unit
is 1 this is the plain bound sum <= 2^n - 1.)"""
import numpy as np

from oracle import c_oracle, grid_ref

H, L, CH, LOG2 = 16, 16, 2, 19
S = 1.0   # log2 of the per-level scale 2
WAVE, WG = 64, 1024
PRIMES = (1, 2654435761, 805459861, 3674653429, 2097192037)
RUN_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 130)
MUTATIONS = ("run_last_dropped", "run_across_cell_change", "pair_row_plus1_on_hashed", "pair_row_xor_on_dense",
             "straddling_second_corner_dropped", "zero_tail_run_not_emitted", "out_of_range_contributes",
             "overflow_entry_lost", "slice_image_not_added", "level_outside_window_written")


def offsets(D=3, align=False, gridtype=0):
    if gridtype == 2:
        return tcnn_offsets(D)
    return grid_ref.make_offsets(D, L, 2.0, H, LOG2, align_corners=align)


def scale_of(level):
    return 16 * 2 ** level - 1


# ---- tiny-cuda-nn's lattice (gridtype 2): resolution = ceil(scale) + 1 = 16 * 2^l; its published grid_index: a dense index
# with stride res over the leading dimensions whose stride is still within the table, the hash where the stride it stopped
# at exceeds the table — in uint32, so at res = 2^16 and above (levels 12..15 here) res^2 wraps to 0, never exceeds the table
# and the level is dense in x and y alone
def tcnn_levels(D):
    out = []
    for l in range(L):
        res = scale_of(l) + 1
        rows = min(-(-res ** D // 8) * 8, 1 << LOG2)
        stride = 1
        for _ in range(D):
            if stride > rows:
                break
            stride = (stride * res) & 0xFFFFFFFF
        out.append((res, rows, rows < stride))
    return out


def tcnn_offsets(D=3):
    return np.concatenate([[0], np.cumsum([r for _, r, _ in tcnn_levels(D)])]).astype(np.int32)


def tcnn_rows(cell, level, D):
    """cell [B, D] int64 lattice coordinates -> level-local row."""
    res, rows, hashed = tcnn_levels(D)[level]
    idx = np.zeros(cell.shape[0], dtype=np.int64)
    if hashed:
        for d in range(D):
            idx ^= (cell[:, d] * PRIMES[d]) & 0xFFFFFFFF
    else:
        s = 1
        for d in range(D):
            if s > rows:
                break
            idx = (idx + cell[:, d] * s) & 0xFFFFFFFF
            s = (s * res) & 0xFFFFFFFF
    return idx % rows


def _lowbit(v):
    return v & -v


def sig_bits_ok(sum_abs, or_abs, bits):
    """sum_abs < 2^bits * (largest power of two dividing every addend), elementwise; addends all zero: true."""
    return (or_abs == 0) | (sum_abs < (_lowbit(or_abs) << bits))


class Case:
    """One input of the table backward on the dyadic lattice.
    M [B, D] int: x = M / 2^k.  gn [L, B, C] int: gradient = gn * 2^-q.  x_bad {point: (dim, value)}: coordinates replaced by
    an out-of-range value (the point then contributes nothing).  neg_zero [L, B, C] bool: zero gradients stored as -0.0.
    window (l0, l1): the levels the call works on."""

    def __init__(self, name, f16, M, k, gn, q, *, gridtype=0, align=False, interp=0, x_bad=None, neg_zero=None,
                 window=(0, L), notes=None):
        self.name, self.f16, self.k, self.q = name, bool(f16), int(k), int(q)
        self.M = np.ascontiguousarray(M, dtype=np.int64)
        self.B, self.D = self.M.shape
        self.gn = np.ascontiguousarray(gn, dtype=np.int64)
        self.C = self.gn.shape[2]
        assert self.gn.shape == (L, self.B, self.C) and self.M.min() >= 0 and self.M.max() <= 2 ** k
        self.gridtype, self.align, self.interp, self.window = gridtype, bool(align), interp, window
        self.off = offsets(self.D, self.align, gridtype)
        self.rows_total = int(self.off[-1])
        self.x = (self.M / 2.0 ** k).astype(np.float32)
        for p, (d, v) in (x_bad or {}).items():
            self.x[p, d] = np.float32(v)
        self.valid = ~np.any((self.x < 0) | (self.x > 1), axis=1)
        self.neg_zero = neg_zero
        self.notes = notes or {}
        self.wbits = k * self.D * (3 if interp == 1 else 1)             # weights are multiples of 2^-wbits
        self.unit_exp = self.wbits + q                                 # one unit = 2^-unit_exp
        self._idx = None

    # ---- inputs
    def grad(self):
        g = (self.gn * 2.0 ** -self.q).astype(np.float16 if self.f16 else np.float32)
        if self.neg_zero is not None:
            assert np.all(self.gn[self.neg_zero] == 0)
            g[self.neg_zero] = -0.0
        return g

    # ---- the lattice, in integers
    def lattice(self, level):
        """(cell [B, D], fraction numerator [B, D] in units 2^-k) of pos = x * scale (+ 0.5)."""
        num = self.M * scale_of(level) + (0 if self.align else 2 ** (self.k - 1))
        return num >> self.k, num & (2 ** self.k - 1)

    def weights(self, level, sel=slice(None)):
        """[B, 2^D] int64 in units 2^-wbits (of the points `sel`)."""
        num = self.M[sel] * scale_of(level) + (0 if self.align else 2 ** (self.k - 1))
        fr = num & (2 ** self.k - 1)
        one = 2 ** self.k
        if self.interp == 1:   # p^2 (3 - 2 p), p = fr / 2^k: fr^2 (3 * 2^k - 2 fr) / 2^3k
            fr = fr * fr * (3 * one - 2 * fr)
            one = one ** 3
        w = np.ones((fr.shape[0], 1 << self.D), dtype=np.int64)
        for c in range(1 << self.D):
            for d in range(self.D):
                w[:, c] *= fr[:, d] if (c >> d) & 1 else one - fr[:, d]
        return w

    def live(self, level):
        """(indices, table rows [n, 2^D], vals [n, 2^D, C]) of the points that contribute on a level."""
        sel = np.flatnonzero(self.valid & np.any(self.gn[level] != 0, axis=1))
        return sel, self.rows(level)[sel] + int(self.off[level]), self.weights(level, sel)[:, :, None] * self.gn[level][sel][:, None, :]

    def rows(self, level):
        """[B, 2^D] level-local rows of the corners."""
        if self.gridtype == 2:
            cell, _ = self.lattice(level)
            out = np.empty((self.B, 1 << self.D), dtype=np.int64)
            for c in range(1 << self.D):
                out[:, c] = tcnn_rows(cell + np.array([(c >> d) & 1 for d in range(self.D)]), level, self.D)
            return out
        if self._idx is None:
            xin = np.where(self.valid[:, None], self.x, np.float32(0.5))
            self._idx = c_oracle.grid_indices(xin, self.off, self.C, S, H, self.gridtype, self.align).astype(np.int64) // self.C
        return self._idx[level]

    def hashed(self, level):
        if self.gridtype == 2:
            return tcnn_levels(self.D)[level][2]
        res = scale_of(level) + 1
        return (res if self.align else res + 1) ** self.D > int(self.off[level + 1] - self.off[level])

    def run_ids(self, level):
        """Maximal stretches of consecutive batch indices of in-range points in one cell: (id per point, head flags)."""
        cell, _ = self.lattice(level)
        same = np.zeros(self.B, dtype=bool)
        same[1:] = np.all(cell[1:] == cell[:-1], axis=1) & self.valid[1:] & self.valid[:-1]
        return np.cumsum(~same) - 1, ~same

    # ---- the reference: integer scatter-add
    def contributions(self, level, mutate=None):
        """(rows [B, 2^D] table rows, vals [B, 2^D, C] int64 units) of one level; `mutate` applies one classic mistake."""
        rows = self.rows(level).copy()
        w = self.weights(level)
        live = self.valid.copy()
        nrows = int(self.off[level + 1] - self.off[level])
        if mutate == "out_of_range_contributes":
            live[:] = True
        vals = w[:, :, None] * self.gn[level][:, None, :] * live[:, None, None]
        rid, head = self.run_ids(level)
        last = np.ones(self.B, dtype=bool)
        last[:-1] = head[1:]
        if mutate == "run_last_dropped":
            vals[last & ~head] = 0
        elif mutate == "run_across_cell_change":   # the first member of a run is added to the rows of the point before it
            sel = np.flatnonzero(head[1:] & self.valid[1:] & self.valid[:-1]) + 1
            rows[sel] = rows[sel - 1]
        elif mutate == "pair_row_plus1_on_hashed" and self.hashed(level):
            rows[:, 1::2] = (rows[:, 0::2] + 1) % nrows
        elif mutate == "pair_row_xor_on_dense" and not self.hashed(level):
            rows[:, 1::2] = rows[:, 0::2] ^ 1
        elif mutate == "straddling_second_corner_dropped":
            vals[:, 1::2][self.pair_codes(level) == 7] = 0
        elif mutate == "zero_tail_run_not_emitted":
            zero = ~np.any(self.gn[level] != 0, axis=1)
            dead = np.zeros(int(rid.max()) + 1, dtype=bool)
            dead[rid[last & zero]] = True
            vals[dead[rid]] = 0
        elif mutate == "overflow_entry_lost":      # one pool entry: one x-neighbour pair of one point
            p = self.notes.get("hot_point", int(np.flatnonzero(live & np.any(self.gn[level] != 0, axis=1))[-1]))
            if level == self.notes.get("hot_level", level):
                vals[p, 0:2] = 0
        elif mutate == "slice_image_not_added":    # a contiguous share of one bucket's entries
            if level == self.notes.get("hot_level", 0):
                b = (rows[:, 0] >> 13) == (rows[self.notes.get("hot_point", 0), 0] >> 13)
                sel = np.flatnonzero(b)
                vals[sel[len(sel) // 2:], 0:2] = 0
        return rows + int(self.off[level]), vals

    def reference(self, mutate=None):
        """The table in int64 units 2^-unit_exp."""
        tab = np.zeros((self.rows_total, self.C), dtype=np.int64)
        l0, l1 = (0, L) if mutate == "level_outside_window_written" else self.window
        for l in range(l0, l1):
            if mutate is None:
                _, rows, vals = self.live(l)
            else:
                rows, vals = self.contributions(l, mutate)
                sel = np.any(vals != 0, axis=(1, 2))
                rows, vals = rows[sel], vals[sel]
            for ch in range(self.C):
                np.add.at(tab[:, ch], rows.ravel(), vals[:, :, ch].ravel())
        return tab

    def to_table(self, units):
        """int64 units -> the table type: the ONE rounding (exact for fp32 under the conditions)."""
        assert np.abs(units).max(initial=0) < 2 ** 53
        return (units.astype(np.float64) * 2.0 ** -self.unit_exp).astype(np.float16 if self.f16 else np.float32)

    def exact(self, units):
        return units.astype(np.float64) * 2.0 ** -self.unit_exp

    # ---- the conditions
    def row_cap_ok(self, bits, per_level=None):
        """per row and channel: the sum of |units| has at most `bits` significant bits above the common unit."""
        if per_level is None:
            per_level = []
            for l in range(*self.window):
                _, rows, vals = self.live(l)
                per_level.append((rows.ravel(), np.abs(vals).reshape(-1, self.C)))
        if not per_level:
            return True
        rows, a = np.concatenate([r for r, _ in per_level]), np.concatenate([v for _, v in per_level])
        order = np.argsort(rows, kind="stable")
        rows, a = rows[order], a[order]
        st = np.flatnonzero(np.concatenate([[True], rows[1:] != rows[:-1]]))
        return bool(np.all(sig_bits_ok(np.add.reduceat(a, st, axis=0), np.bitwise_or.reduceat(a, st, axis=0), bits)))

    def pair_codes(self, level):
        """[B, 2^(D-1)] code of every x-neighbour pair as the plain scatter kernel classes describe it: hashed levels
        trailing ones of the x cell (>= 7: two singles), dense levels 0, or 7 where the pair straddles a 128-row group (or,
        tiny-cuda-nn's lattice, wraps past the level's last row)."""
        rows = self.rows(level)
        r0, r1 = rows[:, 0::2], rows[:, 1::2]
        if self.hashed(level):
            x = r0 ^ r1
            assert np.all((x & (x + 1)) == 0) and np.all(x > 0)   # 2^(t+1) - 1
            t = np.log2(x + 1).astype(np.int64) - 1
            return np.minimum(t, 7)
        code = np.where((r0 & 127) == 127, 7, 0)
        wrap = r1 != r0 + 1
        assert np.all(r1[wrap] == 0)
        return np.where(wrap, 7, code)

    def check_conditions(self):
        assert self.unit_exp <= (24 if self.f16 else 40)         # the fixed-point images hold a unit
        tab = self.reference()
        per_level = []
        for l in range(*self.window):
            sel, rows, vals = self.live(l)
            if not len(sel):
                continue
            num = self.M[sel] * scale_of(l) + (0 if self.align else 2 ** (self.k - 1))
            assert np.all(num // _lowbit(np.maximum(num, 1)) < 2 ** 24), f"{self.name}: C1 fails on level {l}"
            a = np.abs(vals)
            per_level.append((rows.ravel(), a.reshape(-1, self.C)))
            # every contribution (the float product weight * gradient) is exact in float32 / fp16
            assert np.all(a // _lowbit(np.maximum(a, 1)) < 2 ** (11 if self.f16 else 24)), f"{self.name}: (a) fails on level {l}"
            if self.f16:
                assert a.max(initial=0) * 2.0 ** -self.unit_exp <= 65504
                rid = self.run_ids(l)[0][sel]
                st = np.flatnonzero(np.concatenate([[True], rid[1:] != rid[:-1]]))
                assert np.all(sig_bits_ok(np.add.reduceat(a, st, axis=0), np.bitwise_or.reduceat(a, st, axis=0), 11)), \
                    f"{self.name}: (b) fails on level {l}"
        if self.f16:
            t = np.abs(tab)
            assert np.all(t // _lowbit(np.maximum(t, 1)) < 2 ** 24), f"{self.name}: (c) fails"
            assert t.max(initial=0) * 2.0 ** -self.unit_exp <= 65504
        else:
            assert self.row_cap_ok(24, per_level), f"{self.name}: the fp32 row cap fails"
        return tab


# ---- structure of a batch as the scatter kernels see it, from the data alone
def structure(case, level):
    """Per point: continues the run of its lower neighbour (same cell, both members, not at a scan boundary: the wave start,
    and on hashed levels every 16-lane row start).  Members: in-range points with a gradient and those within three lanes
    of one inside their wave (grid_bwd_scatter.hip, "members of runs")."""
    lane = np.arange(case.B) % WAVE
    nz = case.valid & np.any(case.gn[level] != 0, axis=1)
    near = np.zeros(case.B, dtype=bool)
    for s in range(-3, 4):
        sh = np.zeros(case.B, dtype=bool)
        if s >= 0:
            sh[s:] = nz[:case.B - s] & (lane[s:] >= s)
        else:
            sh[:s] = nz[-s:] & (lane[:s] < WAVE + s)
        near |= sh
    member = case.valid & near
    cell, _ = case.lattice(level)
    cont = np.zeros(case.B, dtype=bool)
    cont[1:] = np.all(cell[1:] == cell[:-1], axis=1) & member[1:] & member[:-1]
    cont &= (lane & 15) != 0 if case.hashed(level) else lane != 0
    return member, nz, cont


def emits(case, level):
    """(emit, cont) per point: `cont` after the kMinMerges rule (a wave with fewer than 8 continuing lanes merges nothing),
    `emit` the run tails that send entries to the pool (a zero-gradient run of one sends none)."""
    member, nz, cont = structure(case, level)
    nw = -(-case.B // WAVE)
    c2 = np.pad(cont, (0, nw * WAVE - case.B)).reshape(nw, WAVE)
    cont = (c2 & (c2.sum(axis=1, keepdims=True) >= 8)).ravel()[:case.B]
    nxt = np.zeros(case.B, dtype=bool)
    nxt[:-1] = cont[1:]
    return member & ~nxt & (nz | cont), cont


def plain_entry_buckets(case, level):
    """(workgroup, bucket) of every pool entry of a plain-class level: one per x pair in the bucket of its first row, one
    more in the bucket of its second row where the pair travels as two singles (grid_pool.h)."""
    emit, _ = emits(case, level)
    rows, code = case.rows(level), case.pair_codes(level)
    bucket = (lambda r: r >> 13) if case.hashed(level) else (lambda r: (r >> 7) & 63)
    wg = np.repeat(np.arange(case.B) // WG, 4).reshape(-1, 4)
    b0, b1 = bucket(rows[:, 0::2]), bucket(rows[:, 1::2])
    e0 = np.broadcast_to(emit[:, None], b0.shape)
    e1 = e0 & (code == 7)
    return np.concatenate([wg[e0], wg[e1]]), np.concatenate([b0[e0], b1[e1]])


def batch_runs(case, level):
    """(start index, length) of every maximal same-cell stretch of in-range points."""
    _, head = case.run_ids(level)
    st = np.flatnonzero(head & case.valid)
    rid, _ = case.run_ids(level)
    ln = np.bincount(rid, weights=case.valid.astype(np.float64)).astype(np.int64)[rid[st]]
    return st, ln


# ---- builders
_K2 = np.array([[a, b, c] for a in range(5) for b in range(5) for c in range(5)], dtype=np.int64)   # the 1/4 lattice


def _wmax_k2(M):
    """largest corner weight of a 1/4-lattice point in units 2^-6 (fraction (2 - m) mod 4 on every level)."""
    fr = (2 - M) % 4
    return np.prod(np.maximum(fr, 4 - fr), axis=-1)


def _run_gradients(rng, n, nmax):
    g = rng.integers(1, nmax + 1, (L, n, CH)) * rng.choice([-1, 1], (L, n, CH))
    return g


def _build_runs(name, f16, plan, rng, k=2, extra=None, **kw):
    """plan: list of run lengths laid out back to back; neighbouring runs sit on different 1/4-lattice points (which lie in
    different cells on every level).  Gradient amplitudes are chosen from the fp16 stretch bound (b): |n| <= 2047 // (largest
    corner weight * run length), at most 3."""
    Ms, gs = [], []
    prev = -1
    wm = _wmax_k2(_K2)
    for n in plan:
        ok = np.flatnonzero((wm * n <= 2047) & (np.arange(len(_K2)) != prev))
        prev = int(rng.choice(ok))
        nmax = int(min(3, 2047 // (wm[prev] * n)))
        Ms.append(np.repeat(_K2[prev][None], n, axis=0))
        gs.append(_run_gradients(rng, n, nmax))
    M = np.concatenate(Ms) * 2 ** (k - 2)
    gn = np.concatenate(gs, axis=1)
    if extra is not None:
        M2, g2 = extra
        M, gn = np.concatenate([M, M2]), np.concatenate([gn, g2], axis=1)
    return Case(name, f16, M, k, gn, 4, **kw)


def _run_plan():
    plan = []
    for n in RUN_LENGTHS:
        for _ in range(WAVE):          # period n (odd) or n + 1: 64 repeats start at every lane
            plan.append(n)
            if n % 2 == 0:
                plan.append(1)
    return plan


def case_runs(f16, **kw):
    """1. run-merge position classes: every required length starting at every lane, the row / wave / workgroup crossings.  fp32
    adds 1/32-lattice neighbours that share a cell on level 0 only (a run on one level and not on the next)."""
    rng = np.random.default_rng(101)
    extra, k = None, 2
    if not f16 and not kw:
        k = 5
        n = 4 * WAVE
        M2 = np.tile(np.array([[17, 17, 17], [18, 17, 17]], dtype=np.int64), (n // 2, 1))
        extra = (M2, rng.integers(1, 3, (L, n, CH)) * rng.choice([-1, 1], (L, n, CH)))
    return _build_runs("runs", f16, _run_plan(), rng, k=k, extra=extra, **kw)


def case_runs_small(f16, **kw):
    """Reduced version of 1-3 for the generic classes and the entry-point tests: lengths up to 65 at a few lanes, zero
    stretches, out-of-range points."""
    rng = np.random.default_rng(102)
    plan = []
    for n in (1, 2, 3, 5, 8, 9, 16, 17, 33, 64, 65, 130):
        plan += [n, 1, n, n]
    c = _build_runs("runs_small", f16, plan, rng, **kw)
    return _with_zeros_and_bad(c, rng)


def _with_zeros_and_bad(c, rng):
    st, ln = batch_runs(c, 0)
    gn, bad = c.gn.copy(), {}
    for s, n in zip(st[::3], ln[::3]):
        if n >= 8:
            z = int(rng.integers(1, 9))
            a = s + int(rng.integers(1, n - z)) if n - z > 1 else s
            gn[:, a:a + min(z, n - 1)] = 0
        if n >= 16:
            bad[int(s + n // 2)] = (int(rng.integers(0, 3)), 1.0000001 if rng.random() < 0.5 else -1e-7)
    gn[5, ::7, 0] = 0
    return Case(c.name, c.f16, c.M, c.k, gn, c.q, gridtype=c.gridtype, align=c.align, interp=c.interp, x_bad=bad)


def case_min_merges(f16):
    """2. kMinMerges: waves with exactly 0, 1, 7, 8 and 9 continuing lanes (one run of 1 + c points at the wave's start,
    61 - c.. distinct points behind it)."""
    rng = np.random.default_rng(103)
    plan = []
    for c in (0, 1, 7, 8, 9):
        plan += [1 + c] + [1] * (WAVE - 1 - c)
    return _build_runs("min_merges", f16, plan, rng)


def case_zeros(f16):
    """3. zero and out-of-range samples inside runs."""
    rng = np.random.default_rng(104)
    plan, marks = [], []

    def run(n, what, *a):
        marks.append((sum(plan), n, what) + a)
        plan.append(n)

    for z in range(1, 9):                      # zero stretches of 1..8 inside a run: six are bridged, seven cut it
        run(10 + z, "inner", 5, z)
    for z in (1, 3, 4, 7):
        run(8 + z, "head", z)
        run(8 + z, "tail", z)
    run(12, "all_zero")
    while sum(plan) % WAVE:
        plan.append(1)
    run(WAVE, "all_zero")                      # a whole wave of zeros
    run(12, "neg_zero")
    run(12, "one_channel")
    run(12, "one_level")
    run(20, "bad_hi", 7)
    run(20, "bad_lo", 11)
    c = _build_runs("zeros", f16, plan, rng)
    gn, bad = c.gn.copy(), {}
    negz = np.zeros(gn.shape, dtype=bool)
    for s, n, what, *a in marks:
        if what == "inner":
            gn[:, s + a[0]:s + a[0] + a[1]] = 0
        elif what == "head":
            gn[:, s:s + a[0]] = 0
        elif what == "tail":
            gn[:, s + n - a[0]:s + n] = 0
        elif what == "all_zero":
            gn[:, s:s + n] = 0
        elif what == "neg_zero":               # -0.0 in both channels (no gradient) and in one (a gradient)
            gn[:, s + 2:s + 5] = 0
            negz[:, s + 2:s + 5] = True
            gn[:, s + 7, 1] = 0
            negz[:, s + 7, 1] = True
        elif what == "one_channel":
            gn[:, s + 3:s + 9, 0] = 0
        elif what == "one_level":
            gn[1, s + 4] = 0
            gn[9, s + 5:s + 8] = 0
        elif what == "bad_hi":
            bad[s + a[0]] = (0, 1.0000001)
        elif what == "bad_lo":
            bad[s + a[0]] = (1, -1e-7)
    out = Case("zeros", f16, c.M, c.k, gn, c.q, x_bad=bad, neg_zero=negz)
    out.marks = marks
    return out


def case_pairs(f16):
    """4. pairs and singles: lattice points whose x cell on a hashed level ends in t = 0..6 and >= 7 ones, dense pairs with
    r0 & 127 == 127 beside ordinary ones.  x > 0.5 puts the cell at m * 2^(l+4-k) - 1: t = l + 4 - k + (trailing zeros of m).
    t = 1 on a hashed level (l >= 3) needs k = 6, where pos is exact up to level 14 only — those points carry a zero gradient
    on level 15 (C1 is asserted per (point, level) that carries a gradient).  y and z stay on the 1/2 lattice, so the weights
    keep 6 + 2 bits for fp16."""
    rng = np.random.default_rng(105)
    k = 6
    xs = np.array([33, 34, 35, 36, 40, 44, 48, 52, 56, 60, 63, 64, 0, 8, 16, 24, 32], dtype=np.int64)
    yz = np.array([0, 32, 64], dtype=np.int64)
    M = np.array([[x, y, z] for x in xs for y in yz for z in yz], dtype=np.int64)
    M = M[rng.permutation(len(M))]
    M = np.concatenate([M, M[rng.permutation(len(M))], M[rng.permutation(len(M))][:len(M) - 3]])
    gn = rng.integers(1, 3, (L, len(M), CH)) * rng.choice([-1, 1], (L, len(M), CH))
    odd = (M[:, 0] % 2) == 1
    gn[15, odd] = 0
    return Case("pairs", f16, M, k, gn, 0)


def case_generic(f16, which):
    """6. the generic classes: smoothstep / tiled / align_corners on a reduced version of 1-3, then 1024 + points that merge
    with nobody (more than 6144 staged singles in one workgroup)."""
    kw = {"smoothstep": dict(interp=1), "tiled": dict(gridtype=1), "align": dict(align=True)}[which]
    rng = np.random.default_rng(106)
    k = 1 if (f16 and which == "smoothstep") else 2
    plan = []
    for n in (1, 2, 3, 5, 8, 9, 16, 17, 33, 64, 65):
        plan += [n, 1, n]
    Ms, gs, prev = [], [], -1
    lat = np.array([[a, b, c] for a in range(2 ** k + 1) for b in range(2 ** k + 1) for c in range(2 ** k + 1)], dtype=np.int64)
    for n in plan + [1] * (2 * WG):
        prev = int(rng.choice(np.flatnonzero(np.arange(len(lat)) != prev)))
        Ms.append(np.repeat(lat[prev][None], n, axis=0))
        gs.append(rng.integers(1, 2, (L, n, CH)) * rng.choice([-1, 1], (L, n, CH)))
    c = Case(which, f16, np.concatenate(Ms), k, np.concatenate(gs, axis=1), 2, **kw)
    c.name = which
    return _with_zeros_and_bad(c, rng)


def case_tcnn(f16):
    """5. tiny-cuda-nn's lattice: random 1/4-lattice points and the cells whose x pair starts on a dense level's last row."""
    rng = np.random.default_rng(107)
    M = _K2[rng.integers(0, len(_K2), 1500)]
    # dense levels 0..2 (res 16, 32, 64; rows res^3): the last row is the cell (res-1, res-1, res-1): x = 1 in every
    # dimension puts pos at res - 0.5 -> cell res - 1
    M = np.concatenate([M, np.full((40, 3), 4, dtype=np.int64), _K2[rng.integers(0, len(_K2), 500)]])
    gn = rng.integers(1, 4, (L, len(M), CH)) * rng.choice([-1, 1], (L, len(M), CH))
    return Case("tcnn", f16, M, 2, gn, 4, gridtype=2)


def case_atomic(f16, D, C):
    """11. the atomic entry point: a few hundred points; fp16 keeps per-row sums of |units| within 11 bits, so a running
    fp16 atomic sum is exact in any order."""
    rng = np.random.default_rng(108 + 10 * D + C)
    B = 150 if f16 else 1000
    M = rng.integers(0, 3, (B, D)) * 2 if f16 else rng.integers(0, 5, (B, D))     # fp16: the 1/2 lattice
    gn = rng.integers(-1, 2, (L, B, C)) if f16 else rng.integers(-3, 4, (L, B, C))
    c = Case(f"atomic_D{D}_C{C}", f16, M, 2, gn, 2 if f16 else 4)
    return c


def atomic_fp16_row_cap(case):
    """per row and channel: sum of |units| has at most 11 significant bits above the common unit."""
    return case.row_cap_ok(11)


def case_hot_cell(f16, B, n_hot, seed=109, k=2, nmax=1, x_coarse=False, **kw):
    """7 / 8. the first n_hot points alternate between two cells (so no two neighbours merge), the rest are random lattice
    points: the buckets holding the two cells' rows receive n_hot / 2 entries each on top of their share."""
    rng = np.random.default_rng(seed)
    lat = 2 ** k + 1
    M = rng.integers(0, lat, (B, 3))
    if x_coarse:
        M[:, 0] &= ~1     # x on the coarser lattice: one bit less in every weight (12 -> 11 at k = 4)
    u = 2 ** (k - 2)
    M[0:n_hot:2] = [u, u, u]
    M[1:n_hot:2] = [3 * u, u, 3 * u]
    M[n_hot:][np.all(M[n_hot:] == M[n_hot - 1], axis=1)] = [0, 0, 0]
    # neighbours in the batch must not merge: redraw equal neighbours among the random points
    for _ in range(8):
        eq = np.flatnonzero(np.all(M[1:] == M[:-1], axis=1)) + 1
        eq = eq[eq >= n_hot]
        if not len(eq):
            break
        M[eq, 1:] = rng.integers(0, lat, (len(eq), 2))
    gn = rng.integers(1, nmax + 1, (L, B, CH)) * rng.choice([-1, 1], (L, B, CH))
    return Case("hot_cell", f16, M, k, gn, 0, notes=dict(hot_point=0, hot_level=9), **kw)


def reserved_slots(case, level, plain=True):
    """Pool slots the scatter pass reserves per bucket of a level: the plain kernel rounds every workgroup's count per bucket
    up to an even number (the zero padding entry); the generic kernel sends every corner of an emitting point as a single."""
    if plain:
        wg, bk = plain_entry_buckets(case, level)
        cnt = np.bincount(wg * 64 + bk, minlength=64 * (-(-case.B // WG))).reshape(-1, 64)
        return ((cnt + 1) & ~1).sum(axis=0), cnt
    emit, _ = emits(case, level)
    bk = (case.rows(level)[emit] >> 13).ravel()
    wg = np.repeat(np.flatnonzero(emit) // WG, 8)
    cnt = np.bincount(wg * 64 + bk, minlength=64 * (-(-case.B // WG))).reshape(-1, 64)
    return cnt.sum(axis=0), cnt


def case_overflow_by_a_few(f16, B, cap_of, plain=True, **kw):
    """7. the smallest hot-cell batch whose fullest bucket of one hashed level outgrows its pool slots (cap_of(level), from the
    workspace plan) — on the level whose buckets the random lattice points alone fill least (the lattice is no uniform cloud:
    its hashes fill some levels' buckets quite unevenly).  -> (case, level, slots beyond the pool)."""
    def build(n_hot):
        # plain class: the 1/16 lattice (x on 1/8: 11-bit weights); align_corners has arbitrary fractions: the 1/8 lattice
        return case_hot_cell(f16, B, n_hot, k=3, **kw) if kw.get("align") else case_hot_cell(f16, B, n_hot, k=4, x_coarse=True, **kw)

    base = build(0)
    natural = {l: int(reserved_slots(base, l, plain)[0].max()) - cap_of(l) for l in range(3, L)}
    level = min(natural, key=natural.get)
    assert natural[level] < 0, natural

    def over(n_hot):
        c = build(n_hot)
        return c, int(reserved_slots(c, level, plain)[0].max()) - cap_of(level)
    lo, hi = 0, B // 2            # pairs of hot points
    assert over(2 * hi)[1] >= 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if over(2 * mid)[1] >= 1 else (mid, hi)
    c, ov = over(2 * hi)
    c.notes["hot_level"] = level
    return c, level, ov


def case_unstaged(f16):
    """7. a workgroup whose entries exceed its staging area: x = 1 puts the x cell of every hashed level at 16 * 2^l - 1
    (seven or more trailing ones): every pair travels as two singles, eight entries per point where nobody merges — 8192
    against the 5120 staging slots of a plain workgroup."""
    rng = np.random.default_rng(110)
    B = 2 * WG
    M = rng.integers(0, 9, (B, 3))
    M[:, 0] = 8
    for _ in range(8):
        eq = np.flatnonzero(np.all(M[1:] == M[:-1], axis=1)) + 1
        M[eq, 1:] = rng.integers(0, 9, (len(eq), 2))
    gn = rng.integers(1, 3, (L, B, CH)) * rng.choice([-1, 1], (L, B, CH))
    return Case("unstaged", f16, M, 3, gn, 0)


def unstaged_facts(case, level, cap_stage=5 * WG):
    """(a workgroup stages more than cap_stage entries, some bucket's padding entry lies beyond the staging area)."""
    _, cnt = reserved_slots(case, level)
    ev = (cnt + 1) & ~1
    end = np.cumsum(ev, axis=1)
    return bool(np.any(end[:, -1] > cap_stage)), bool(np.any((cnt % 2 == 1) & (end - 1 >= cap_stage)))


def case_spill_full():
    """8. fp32: HALF of 320 K points in one cell at x = 1, the other half outside the grid (no two neighbours merge): the hashed buckets
    holding the cell's rows overflow their pools and the level's spill list; the rest goes into the table with float
    atomics — exact all the same: the 1/4 lattice with |n| = 1 keeps every row's sum of |units| under 2^24."""
    rng = np.random.default_rng(111)
    B = 320 * 1024
    M = np.ones((B, 3), dtype=np.int64)
    M[:, 0] = 4      # x = 1: every pair of a hashed level travels as two singles, eight entries per point
    gn = rng.choice([-1, 1], (L, B, CH))
    c = Case("spill_full", False, M, 2, gn, 0)
    c.x[1::2] = np.float32(1.5)
    c.valid = ~np.any((c.x < 0) | (c.x > 1), axis=1)
    return c


def case_chunked(f16, B, n_live=250):
    """10. a batch the minimum workspace walks in several chunks: `n_live` samples spread over the whole batch carry a
    gradient, the rest carry none and are dropped — per row the sum of |units| over ALL chunks stays within 11 bits, so the
    fp16 table's rounding after every chunk is the identity."""
    rng = np.random.default_rng(112)
    M = rng.integers(0, 5, (B, 3))
    gn = np.zeros((L, B, CH), dtype=np.int64)
    live = np.sort(rng.choice(B, n_live, replace=False))
    live[0], live[-1] = 0, B - 1
    gn[:, live] = rng.choice([-1, 1], (L, n_live, CH))
    return Case("chunked", f16, M, 2, gn, 2)
