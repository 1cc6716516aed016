"""Known-answer tests of the occupancy-grid marchers, through the C ABI: lnh_march_rays_train (one wave per ray, 64 lattice
points a chunk; a pending exit, the max_steps cap and last_t carried between chunks), lnh_march_rays_train_ordered (the same
walk, rows in ray order), lnh_lidar_march_rays (a second copy of the chunk loop with a per-round budget and a resume
parameter) and the serial template lnh_march_rays.

The expected samples come from tests/march_exact_cases.py: an exact model of the serial walk (fractions over the float32
inputs; only the lattice recurrence is float32) on cases whose every float32 decision keeps 8 times its rounding error from
the alternative — asserted, with the coverage of the case list and the teeth of the construction, by
tests/test_march_exact_cpu.py without a GPU.  So every comparison here is torch.equal / assert_array_equal on bits: counts,
ray tables, deltas, dirs, resume parameters; xyzs equal the C oracle's bits AND are correctly rounded clip(o + t d).
Discipline of tests/exact_util.py: sentinel-filled outputs with guard words, NaN rows behind every float input, zero padding
behind the bitfield, every call twice.  No deliberately wrong kernel is built or run for this suite: the mistakes live in the
CPU emulator only (a wrong walk may not terminate).

MEASURED on an MI355X: 171 tests in 11.2 s (about 5 s of it the exact model on the host), slowest test 1.2 s (the alive loop of
`rows8` in 591 rounds of one sample); tests/test_ragged_exact_gpu.py: 330 tests in 6.5 s.  No kernel needed a change.
"""

import numpy as np
import pytest
import torch

import march_exact_cases as mc
from exact_util import GUARD, SENT, Out, _poisoned
from oracle import c_oracle

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = mc.case_names()
I32 = torch.int32


def _call(name, *args):
    from gpu_util import call
    call(name, *[a.buf if isinstance(a, Out) else a for a in args])


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _in(a, row_len):
    return _poisoned(_f32(a), row_len)


def _filled(values, dt):
    values = np.asarray(values)
    o = Out(values.shape, dt)
    o.data().copy_(torch.from_numpy(np.ascontiguousarray(values)).cuda().to(dt))
    return o


def _bits(t):
    return t.view(I32) if t.dtype == torch.float32 else t


def _same(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _untouched(*outs):
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.buf == SENT).all()), "a refused or empty call wrote to an output"


class Problem:
    """A case on the device, with what the model expects of it (computed once per case and kept)."""
    _cache = {}

    def __init__(self, c):
        self.c, g = c, c.grid
        o, d, near, far, noise = c.arrays()
        self.host = (o, d, near, far, noise)
        self.o, self.d = _in(o, 3), _in(d, 3)
        self.near, self.far, self.noise = _in(near, 1), _in(far, 1), _in(noise, 1)
        self.bits = torch.zeros(g.bits.size + 64, dtype=torch.uint8, device="cuda")
        self.bits[:g.bits.size] = torch.from_numpy(g.bits).cuda()
        self.geo = (g.bound, c.dt_gamma, c.max_steps)
        walks = mc.march_model(c)
        self.counts = np.array([len(w.idx) for w in walks], np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)])
        self.total = int(self.offsets[-1])
        self.deltas = np.concatenate([mc.expected_rows(c, n, w.idx) for n, w in enumerate(walks)] + [np.zeros((0, 2), F)])
        self.dirs = np.repeat(d, self.counts, axis=0)
        # xyzs: the C oracle's bits (its counts are the model's: tests/test_march_exact_cpu.py, and again here), which must
        # also be correctly rounded clip(o + t d) in the model's exact arithmetic
        cap = c.cap_override
        if cap is None:
            x, _, _, rays, _ = c_oracle.march_rays_train(o, d, g.bits, g.bound, c.dt_gamma, c.max_steps, g.C, g.H, self.total + 1,
                                                         near, far, noise)
            np.testing.assert_array_equal(rays[:, 2], self.counts)
            self.xyzs = x[:self.total]
        else:
            x, _, _ = c_oracle.march_rays(c.N, cap, np.arange(c.N), near, o, d, g.bound, c.dt_gamma, c.max_steps, g.C, g.H, g.bits,
                                          near, far, noise)
            self.xyzs = np.concatenate([x[n * cap:n * cap + k] for n, k in enumerate(self.counts)] + [np.zeros((0, 3), F)])
        for n, w in enumerate(walks):
            b = int(self.offsets[n])
            assert mc.xyz_is_correctly_rounded(c, n, w.idx, self.xyzs[b:b + len(w.idx)]), (c.name, n)

    @classmethod
    def get(cls, c):
        if c.name not in cls._cache:
            cls._cache[c.name] = cls(c)
        return cls._cache[c.name]

    def rows(self, table, M):
        """Expected (xyzs, dirs, deltas) of M rows for a ray table [(id, offset, count)]: the rows of every ray that fits
        at its offset, the sentinel everywhere else."""
        x, dr, dl = np.full((M, 3), SENT, F), np.full((M, 3), SENT, F), np.full((M, 2), SENT, F)
        for rid, off, cnt in table:
            if cnt and off + cnt <= M:
                b = int(self.offsets[rid])
                x[off:off + cnt], dr[off:off + cnt], dl[off:off + cnt] = self.xyzs[b:b + cnt], self.dirs[b:b + cnt], self.deltas[b:b + cnt]
        return x, dr, dl


def _train(fn, p, M, N=None, C=None, max_steps=None, null=None, outs=None):
    c, g = p.c, p.c.grid
    N = c.N if N is None else N
    if outs is None:
        outs = (Out((M, 3), torch.float32), Out((M, 3), torch.float32), Out((M, 2), torch.float32), Out((c.N, 3), I32),
                _filled(np.zeros(2, np.int32), I32))
    a = [p.o, p.d, p.bits, g.bound, c.dt_gamma, c.max_steps if max_steps is None else max_steps, N, g.C if C is None else C, g.H,
         M, p.near, p.far, outs[0], outs[1], outs[2], outs[3], outs[4], p.noise]
    if null is not None:
        a[null] = None
    _call(fn, *a)
    return outs


def _check_rows(p, outs, table, M, what):
    _check_bits(outs, p.rows(table, M), what)


def _check_bits(outs, want, what):
    """xyzs, dirs, deltas against the expected arrays BIT for bit (rows nobody owns keep the sentinel), guard words intact."""
    for o, w, k in zip(outs, want, ("xyzs", "dirs", "deltas")):
        assert bool((o.buf[o.n:] == SENT).all()), f"{what}: guard words behind {k} were overwritten"
        got, w = o.data().view(I32), _f32(w).view(I32)
        if not torch.equal(got, w):
            bad = (got != w).nonzero()
            raise AssertionError(f"{what}: {k}: {len(bad)} of {w.numel()} words differ, first at row {bad[0].tolist()}")


# ================================================================================================ the training marchers
@pytest.mark.parametrize("name", NAMES)
def test_march_rays_train(name):
    """Arrival order: the ray table keyed by ray id — every id once, the model's count, disjoint spans that tile
    [0, sum of counts) — counter == (sum, N), and for EVERY ray its rows of xyzs, dirs and deltas; twice."""
    p = Problem.get(mc.cases()[name])
    N, M = p.c.N, p.total + 8
    for rep in range(2):
        outs = _train("lnh_march_rays_train", p, M)
        torch.cuda.synchronize()
        table = outs[3].data().cpu().numpy()
        assert bool((outs[3].buf[outs[3].n:] == SENT).all()) and bool((outs[4].buf[2:] == SENT).all())
        np.testing.assert_array_equal(np.sort(table[:, 0]), np.arange(N))
        np.testing.assert_array_equal(table[:, 2], p.counts[table[:, 0]])
        by_offset = table[np.argsort(table[:, 1], kind="stable")]
        by_offset = by_offset[by_offset[:, 2] > 0]
        np.testing.assert_array_equal(by_offset[:, 1], np.concatenate([[0], np.cumsum(by_offset[:, 2])])[:-1])
        assert outs[4].data().tolist() == [p.total, N]
        _check_rows(p, outs, table, M, f"{name} call {rep}")


@pytest.mark.parametrize("name", NAMES)
def test_march_rays_train_ordered(name):
    """Ray order: the whole output — offsets are the exclusive scan of the model's counts, every ray's rows the bits the
    arrival-order marcher gives it (both equal the expected rows).  At M = total and M = total - 1 the dropped rays are
    exactly those with offset + count > M; their table entry stays and no row is written for them."""
    p = Problem.get(mc.cases()[name])
    N = p.c.N
    table = np.stack([np.arange(N), p.offsets[:-1], p.counts], 1)
    for M in (p.total + 8, p.total, p.total - 1):
        if M < 1:
            continue
        first = None
        for rep in range(2):
            outs = _train("lnh_march_rays_train_ordered", p, M)
            outs[3].check(torch.from_numpy(table.astype(np.int32)).cuda(), f"{name} M = {M}: ray table")
            outs[4].check(torch.tensor([p.total, N], dtype=I32, device="cuda"), f"{name} M = {M}: counter")
            _check_rows(p, outs, table, M, f"{name} M = {M}")
            if first is not None:
                assert all(_same(u.buf, v.buf) for u, v in zip(first, outs)), "two identical calls gave different bits"
            first = outs
        if M == p.total - 1:
            dropped = [n for n in range(N) if p.counts[n] and p.offsets[n] + p.counts[n] > M]
            assert dropped == [int(np.nonzero(p.counts)[0][-1])]
    # the two marchers against each other, ray by ray: the arrival-order rows gathered into ray order
    arrival, ordered = _train("lnh_march_rays_train", p, p.total + 8), _train("lnh_march_rays_train_ordered", p, p.total + 8)
    torch.cuda.synchronize()
    t = arrival[3].data().cpu().numpy()
    t = t[np.argsort(t[:, 0], kind="stable")]
    src = torch.from_numpy(np.concatenate([np.arange(off, off + cnt) for _, off, cnt in t] + [np.zeros(0, np.int64)]).astype(np.int64)).cuda()
    for a, o, k in zip(arrival[:3], ordered[:3], ("xyzs", "dirs", "deltas")):
        assert torch.equal(a.data().view(I32)[src], o.data().view(I32)[:p.total]), f"{name}: {k} of the two marchers differ"


def test_train_refusals_and_no_rays():
    """N = 0 returns; max_steps = 0, C = 9, C = 0 and a null pointer raise.  Every output byte stays as it was."""
    p = Problem.get(mc.cases()["coarse16"])
    M = p.total + 8
    for fn in ("lnh_march_rays_train", "lnh_march_rays_train_ordered"):
        outs = (Out((M, 3), torch.float32), Out((M, 3), torch.float32), Out((M, 2), torch.float32), Out((p.c.N, 3), I32), Out((2,), I32))
        _train(fn, p, M, N=0, outs=outs)
        for kw in (dict(max_steps=0), dict(C=9), dict(C=0)):
            with pytest.raises(RuntimeError, match="bad cascade"):
                _train(fn, p, M, outs=outs, **kw)
        for null in (0, 2, 10, 12, 15, 16, 17):                  # rays_o, grid, nears, xyzs, rays, counter, noises
            with pytest.raises(RuntimeError, match="null pointer"):
                _train(fn, p, M, null=null, outs=outs)
        _untouched(*outs)


# ================================================================================================ the alive-ray marcher
def _padded(p):
    """Per-ray padded device tables of the expected samples: xyz [N, K, 3], deltas [N, K, 2], the bits of the lattice point
    behind sample k [N, K]."""
    c, K = p.c, max(int(p.counts.max()), 1)
    X, D, T = np.zeros((c.N, K, 3), F), np.zeros((c.N, K, 2), F), np.zeros((c.N, K), np.int32)
    for n, w in enumerate(mc.march_model(c)):
        b, k = int(p.offsets[n]), len(w.idx)
        X[n, :k], D[n, :k] = p.xyzs[b:b + k], p.deltas[b:b + k]
        lat = mc.case_ray(c, n).lat
        T[n, :k] = np.array([lat.T(i + 1) for i in w.idx], F).view(np.int32)
    return _f32(X), _f32(D), torch.from_numpy(T).cuda(), torch.from_numpy(p.counts).cuda(), K


def _guarded(t):
    buf = torch.full((t.numel() + GUARD,), SENT, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = t
    return buf


@pytest.mark.parametrize("n_step", mc.N_STEPS_LIDAR)
@pytest.mark.parametrize("name", NAMES)
def test_lidar_march_rays_rounds(name, n_step):
    """The alive loop on the case with noise 0, as many rounds as the model says, the survivors picked by the test from
    rays_t (no compositor).  After EVERY round: the table (id, slot * n_step, count) and empty rows behind the alive count,
    the samples of every slot = the next samples of the model, 0 in unfilled delta slots and the sentinel in unfilled xyz
    slots, rays_steps = the running total, rays_t = the bits of the next lattice point or +inf exactly where the model says
    the ray ended or holds max_steps; both of two identical calls.  samples_total: null for odd n_step, else the round's
    sum.  Everything stays on the device (no synchronisation inside the loop); the flags are read at the end."""
    c = mc.lidar_case(name)
    p = Problem.get(c)
    g, N, ms = c.grid, c.N, c.max_steps
    X, D, T, cnt, K = _padded(p)
    n_rounds = len(mc.lidar_rounds_model(c, n_step))
    ar = torch.arange(N, device="cuda")
    k = torch.arange(n_step, device="cuda")[None]
    inf = torch.full((N,), mc.INF_BITS, dtype=I32, device="cuda")
    t_buf = _guarded(_f32(p.host[2]))
    s_buf = _guarded(torch.zeros(N, dtype=I32, device="cuda"))
    with_total = n_step % 2 == 0
    fresh = [Out((N * n_step, 3), torch.float32).buf, Out((N * n_step, 2), torch.float32).buf, Out((N, 3), I32).buf,
             _filled(np.zeros(1, np.int32), I32).buf]           # sentinel-filled outputs with guard words; the counter starts at 0
    ok = {w: torch.ones((), dtype=torch.bool, device="cuda") for w in
          ("twice", "table", "deltas", "xyzs", "rays_steps", "rays_t", "guards", "samples_total")}
    for _ in range(n_rounds + 1):                                # one more: nobody is alive, the call writes empty rows only
        dead = t_buf[:N].view(I32) == mc.INF_BITS
        alive_count = (~dead).sum().to(I32).reshape(1)
        ids = torch.argsort(dead.to(torch.int8), stable=True)     # the alive ids in ascending order, then the dead ones
        m = ar < alive_count
        before = s_buf[:N].long()[ids]
        take = torch.where(m, (cnt[ids] - before).clamp(min=0, max=n_step), torch.zeros_like(before))
        total = before + take
        runs, ids32 = [], ids.to(I32)
        for _rep in range(2):
            tb, sb = t_buf.clone(), s_buf.clone()
            x, dl, table, tot = (b.clone() for b in fresh)
            _call("lnh_lidar_march_rays", N, n_step, N, alive_count, ids32, tb, sb, p.o, p.d, p.bits, g.bound, c.dt_gamma, ms,
                  g.C, g.H, p.far, x, dl, table, tot if with_total else None)
            runs.append((tb, sb, x, dl, table, tot))
        ok["twice"] &= torch.stack([(_bits(u) == _bits(v)).all() for u, v in zip(*runs)]).all()
        tb, sb, xb, dlb, tab, totb = runs[0]
        want_table = torch.stack([torch.where(m, ids, 0), torch.where(m, ar * n_step, 0), take], 1).to(I32)
        ok["table"] &= (tab[:N * 3].view(N, 3) == want_table).all()
        v = (k < take[:, None])[..., None]
        src = (before[:, None] + k).clamp(max=K - 1)
        want_dl = torch.where(v, D[ids[:, None], src], torch.zeros((), device="cuda"))
        want_x = torch.where(v, X[ids[:, None], src], torch.full((), SENT, device="cuda"))
        ok["deltas"] &= (dlb[:N * n_step * 2].view(I32) == want_dl.reshape(-1).view(I32)).all()
        ok["xyzs"] &= (xb[:N * n_step * 3].view(I32) == want_x.reshape(-1).view(I32)).all()
        want_s = s_buf[:N].clone()
        want_s[ids] = torch.where(m, total, before).to(I32)
        ok["rays_steps"] &= (sb[:N] == want_s).all()
        mark = torch.where((take == n_step) & (total < ms), T[ids, (total - 1).clamp(min=0)], inf)
        want_t = t_buf[:N].view(I32).clone()
        want_t[ids] = torch.where(m, mark, want_t[ids])
        ok["rays_t"] &= (tb[:N].view(I32) == want_t).all()
        ok["guards"] &= torch.stack([(b[-GUARD:] == SENT).all() for b in (tb, sb, xb, dlb, tab)]).all() & (totb[1:] == SENT).all()
        ok["samples_total"] &= totb[0] == (take.sum().to(I32) if with_total else 0)
        t_buf, s_buf = tb, sb
    torch.cuda.synchronize()
    failed = [w for w, f in ok.items() if not bool(f)]
    assert not failed, f"{name}, n_step {n_step}, {n_rounds} rounds: {failed} differ from the model"
    assert bool((t_buf[:N].view(I32) == mc.INF_BITS).all()), "a ray is still alive after the model's last round"
    np.testing.assert_array_equal(s_buf[:N].cpu().numpy(), p.counts)


def test_lidar_refusals_and_no_rays():
    """N = 0 returns; n_step = 0, max_steps = 0, C = 9, n_alive_max > N and null pointers raise.  No output byte changes."""
    c = mc.lidar_case("coarse16")
    p = Problem.get(c)
    g, N, n_step = c.grid, c.N, 4
    outs = (Out((N,), torch.float32), Out((N,), I32), Out((N * n_step, 3), torch.float32), Out((N * n_step, 2), torch.float32),
            Out((N, 3), I32), Out((1,), I32))
    count, ids = torch.tensor([N], dtype=I32, device="cuda"), torch.arange(N, dtype=I32, device="cuda")

    def call(n_alive_max=N, n_step=n_step, N_=N, max_steps=c.max_steps, C=g.C, null=None):
        a = [n_alive_max, n_step, N_, count, ids, outs[0], outs[1], p.o, p.d, p.bits, g.bound, c.dt_gamma, max_steps, C, g.H, p.far,
             outs[2], outs[3], outs[4], outs[5]]
        if null is not None:
            a[null] = None
        _call("lnh_lidar_march_rays", *a)
    call(n_alive_max=0, N_=0)
    for kw, msg in ((dict(n_step=0), "n_step"), (dict(max_steps=0), "bad cascade"), (dict(C=9), "bad cascade"),
                    (dict(n_alive_max=N + 1), "n_alive_max"), (dict(null=5), "null ray state"), (dict(null=6), "null ray state"),
                    (dict(null=3), "null pointer"), (dict(null=9), "null pointer"), (dict(null=16), "null pointer"),
                    (dict(null=18), "null pointer")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    _untouched(*outs)


# ================================================================================================ the serial template
@pytest.mark.parametrize("n_step,noise", mc.SERIAL_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_march_rays_serial_template(name, n_step, noise):
    """lnh_march_rays, single calls: every ray from a lattice point of its own walk (rays_t, indexed by ray id; the alive
    list is the ids in reverse), perturbed by `noise`, at most n_step samples — the model's samples from that start; the
    slots a ray does not fill keep the sentinel."""
    c = mc.serial_case(name, n_step, noise)
    p = Problem.get(c)
    g, N = c.grid, c.N
    alive = torch.arange(N - 1, -1, -1, dtype=I32, device="cuda")
    table = [(N - 1 - s, s * n_step, int(p.counts[N - 1 - s])) for s in range(N)]
    first = None
    for rep in range(2):
        outs = (Out((N * n_step, 3), torch.float32), Out((N * n_step, 3), torch.float32), Out((N * n_step, 2), torch.float32))
        _call("lnh_march_rays", N, n_step, alive, p.near, p.o, p.d, g.bound, c.dt_gamma, c.max_steps, g.C, g.H, p.bits, p.near, p.far,
              outs[0], outs[1], outs[2], p.noise)
        # expected: the rows of slot s at s * n_step, everything else untouched
        x, dr, dl = np.full((N * n_step, 3), SENT, F), np.full((N * n_step, 3), SENT, F), np.full((N * n_step, 2), SENT, F)
        for rid, off, k in table:
            b = int(p.offsets[rid])
            x[off:off + k], dr[off:off + k], dl[off:off + k] = p.xyzs[b:b + k], p.dirs[b:b + k], p.deltas[b:b + k]
        _check_bits(outs, (x, dr, dl), c.name)
        if first is not None:
            assert all(_same(u.buf, v.buf) for u, v in zip(first, outs)), "two identical calls gave different bits"
        first = outs


def test_serial_refusals_and_no_rays():
    """n_alive = 0 and n_step = 0 return; max_steps = 0, a cascade beyond the entry point's limit (16 for this one) and a null
    pointer raise.  No output byte changes."""
    c = mc.serial_case("coarse16", 64, 0.0)
    p = Problem.get(c)
    g, N, n_step = c.grid, c.N, 64
    outs = (Out((N * n_step, 3), torch.float32), Out((N * n_step, 3), torch.float32), Out((N * n_step, 2), torch.float32))
    alive = torch.arange(N, dtype=I32, device="cuda")

    def call(n_alive=N, n_step=n_step, max_steps=c.max_steps, C=g.C, null=None):
        a = [n_alive, n_step, alive, p.near, p.o, p.d, g.bound, c.dt_gamma, max_steps, C, g.H, p.bits, p.near, p.far, outs[0], outs[1],
             outs[2], p.noise]
        if null is not None:
            a[null] = None
        _call("lnh_march_rays", *a)
    call(n_alive=0)
    call(n_step=0)
    for kw in (dict(max_steps=0), dict(C=17), dict(C=0)):
        with pytest.raises(RuntimeError, match="bad cascade"):
            call(**kw)
    for null in (2, 3, 11, 14, 16, 17):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(null=null)
    _untouched(*outs)
