"""Known-answer tests of the optimizer step (csrc/optim.hip) through the C ABI: lnh_grad_check_f16, lnh_adam_table_step,
lnh_adam_table_step_dlr, lnh_train_check, lnh_train_step, lnh_zero_regions.

Problems, references and the bound: tests/optim_exact_cases.py (conditions asserted on the CPU by tests/test_optim_exact_cpu.py;
DESIGN.md section 8, "Exact tests of the optimizer step").  TIER A: exp_avg, exp_avg_sq, the parameters and their fp16 copy are
compared bit for bit with the float32 restatement, `state` as integers after every call.  Where a power of the double pow is
not exact (production betas at t >= 2) step_size and bc2_sqrt may each be the reference float or a neighbour, and ONE of the nine
pairs must give the whole parameter array; the learning rate inside the schedule is held to one ulp.  TIER B: the same runs
against Adam in float64, |p - p64| <= sum over the steps of K(s) 2^-24 A(s), K counted on the kernel text; the test prints the
largest multiple it sees.  Discipline of tests/exact_util.py: sentinel words behind every written buffer, NaN words behind every
gradient, every run made twice with equal bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_exact_cases as oc
from exact_util import GUARD, POISON_ROWS, SENT, Out

pytestmark = pytest.mark.gpu
F32 = np.float32
EPS = oc.EPS
SCALING = (2.0, 0.5)   # growth, back-off
_TORCH = {np.float32: torch.float32, np.float16: torch.float16}


def _call(name, *args):
    from gpu_util import call
    call(name, *args)


def _H():
    from lidarnerf import _hip
    return _hip


def _cast(a):
    return C.cast(a, C.c_void_p)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _io(a):
    """A buffer the kernels write: the values, then GUARD sentinel words."""
    a = np.ascontiguousarray(a)
    o = Out(a.shape, _TORCH[a.dtype.type])
    if a.size:
        o.data().copy_(_up(a))
    return o


def _grad16(bits):
    """fp16 gradient from raw patterns, NaN words behind it."""
    return _up(np.concatenate([np.asarray(bits, np.uint16), np.full(POISON_ROWS, 0x7e00, np.uint16)]).view(np.float16))


def _grad32(a):
    return _up(np.concatenate([np.asarray(a, F32), np.full(POISON_ROWS, np.nan, F32)]))


def _ibits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _host(buf, n):
    return buf[:n].cpu().numpy()


def _same(buf, want, what):
    """`buf` (a snapshot of an Out's storage) holds exactly the bits of `want`, and its guard words."""
    want = np.ascontiguousarray(want)
    n = want.size
    assert buf.numel() == n + GUARD and bool((buf[n:] == SENT).all()), f"{what}: guard words behind the buffer were overwritten"
    got, w = _ibits(buf[:n]), _ibits(_up(want.reshape(-1)))
    if not torch.equal(got, w):
        bad = (got != w).nonzero().view(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {n} elements differ, first at {i}: got {buf[i].item()!r} "
                             f"({int(got[i]) & 0xffffffff:#x}), want {want.reshape(-1)[i]!r}")


def _equal_snaps(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_ibits(a[k]), _ibits(b[k])), f"{what}: {k} differs"


# ================================================================================================ the device side
class Rig:
    """Table buffers of n elements (a window of the shared inputs), the sixteen small tensors, the state."""

    def __init__(self, n, off=1, state=None):
        self.n, self.off = n, off
        self.P, self.M, self.V = _io(oc.table_params()[off:off + n]), _io(np.zeros(n, F32)), _io(np.zeros(n, F32))
        self.P16 = Out((n,), torch.float16)
        self.st = _io(oc.new_state(IT_NEXT=oc.ITERS) if state is None else state)
        ps, ms, vs = oc.small_inputs()
        self.Q, self.SM, self.SV = [_io(p) for p in ps], _io(np.concatenate(ms)), _io(np.concatenate(vs))
        H = _H()
        self.pp = H.ptr_array([q.buf.data_ptr() for q in self.Q])
        self.nn = H.u32_array(oc.SMALL_NUMEL)

    def outs(self):
        d = {"p": self.P, "m": self.M, "v": self.V, "p16": self.P16, "state": self.st, "sm": self.SM, "sv": self.SV}
        d.update({f"q{k}": q for k, q in enumerate(self.Q)})
        return d

    def snap(self):
        return {k: o.buf.clone() for k, o in self.outs().items()}

    def grads(self, k, bad=None):
        """Gradients of call k on the device: (table, [small], pointer array).  bad: 'table' / 'small' puts one inf in."""
        bits = oc.table_grad(k)[self.off:self.off + self.n].copy()
        sg = [None if g is None else g.copy() for g in oc.small_grads(k)]
        if bad == "table":
            bits[self.n // 2] = 0x7c00
        elif bad == "small":
            sg[7][16400] = np.inf
        G, SG = _grad16(bits), [None if g is None else _grad32(g) for g in sg]
        return G, SG, _H().ptr_array([None if g is None else g.data_ptr() for g in SG])

    def check(self, G, n16, gp, n_small=16, div_table=1.0, div_small=oc.DIV_SMALL, lr0=oc.LR0, iters=oc.ITERS):
        _call("lnh_train_check", self.st.buf, G, n16, _cast(gp), _cast(self.nn), n_small, div_table, div_small, lr0, iters)

    def step(self, G, gp, betas=oc.PROD_BETAS, interval=2000, table=True):
        t = (self.P.buf, self.M.buf, self.V.buf, G, self.P16.buf, self.n) if table else (None, None, None, None, None, 0)
        _call("lnh_train_step", self.st.buf, *t, _cast(self.pp), _cast(gp), _cast(self.nn), 16, self.SM.buf, self.SV.buf,
              *betas, EPS, *SCALING, interval)


def execute(run, entry):
    """Every call of a run through one entry point: snapshots of all buffers after each call."""
    scale, div_table = oc.INV_SOURCE[run.inv]
    rig = Rig(run.n, run.off, oc.new_state(scale, IT_NEXT=oc.ITERS))
    snaps = []
    if entry == "train_step":
        for k, stepped in enumerate(run.steps):
            G, SG, gp = rig.grads(k, None if stepped else "table")
            rig.check(G, run.n, gp, div_table=div_table)
            mid = rig.st.buf.clone()
            rig.step(G, gp, run.betas)
            snaps.append(dict(rig.snap(), state_check=mid))
        return snaps
    inv, lr = _up(np.array([oc.INVS[run.inv]], F32)), _up(np.array([run.lr], F32))
    steps = [_io(np.zeros(1, F32)), _io(np.zeros(1, F32))]
    for k, stepped in enumerate(run.steps):
        G, _, _ = rig.grads(k, None if stepped else "table")
        found = _io(np.zeros(1, F32))
        _call("lnh_grad_check_f16", G, run.n, found.buf)
        args = (rig.P.buf, rig.M.buf, rig.V.buf, G, rig.P16.buf, run.n)
        tail = (*run.betas, EPS, inv, found.buf, steps[k % 2].buf, steps[1 - k % 2].buf)
        if entry == "adam":
            _call("lnh_adam_table_step", *args, run.lr, *tail)
        else:
            _call("lnh_adam_table_step_dlr", *args, lr, *tail)
        s = rig.snap()
        snaps.append({"p": s["p"], "m": s["m"], "v": s["v"], "p16": s["p16"], "found": found.buf.clone(),
                      "t": steps[1 - k % 2].buf.clone()})
    return snaps


def verify(run, entry, snaps):
    """Tier A on every call, then tier B on the parameters.  Returns the matched scalar pair of every stepped call."""
    n, what = run.n, f"{run.name} [{entry}]"
    train = entry == "train_step"
    scale, div_table = oc.INV_SOURCE[run.inv]
    p0, grads = oc.run_inputs(run)
    p, m, v, t = p0.copy(), np.zeros(n, F32), np.zeros(n, F32), 0
    p16 = np.full(n, SENT, np.float16)
    st = oc.new_state(scale, IT_NEXT=oc.ITERS)
    ps, ms, vs = oc.small_inputs()
    q, sm, sv = [a.copy() for a in ps], np.concatenate(ms), np.concatenate(vs)
    matched, stepped_p, invs = [], [], []
    for k, (g, stepped, snap) in enumerate(zip(grads, run.steps, snaps)):
        w = f"{what} call {k}"
        lr, inv, inv_small = run.lr, oc.INVS[run.inv], None
        if train:
            a = oc.train_check(st, not stepped, div_table, oc.DIV_SMALL, oc.LR0, oc.ITERS)
            _same(snap["state_check"], a, w + " state after the check")
            st, skip = oc.train_step(a)
            _same(snap["state"], st, w + " state after the step")
            assert skip == (not stepped) and (a[oc.INV_TABLE] == inv or not all(run.steps[:k]))
            lr, inv, inv_small = float(a[oc.LR]), a[oc.INV_TABLE], a[oc.INV]   # (a skipped call has halved the scale)
        else:
            assert _host(snap["found"], 1)[0] == (0.0 if stepped else 1.0), w + ": lnh_grad_check_f16"
        if stepped:
            t += 1
            m, v = oc.moments_f32(m, v, oc.unscale(g, inv), *run.betas)
            got = _host(snap["p"], n)
            exact = t == 1 or run.betas == oc.EXACT_BETAS
            cands = oc.candidates(lr, *run.betas, t)
            for label, s, b in cands[:1] if exact else cands:
                p1, p16_1 = oc.param_f32(p, m, v, s, b)
                if np.array_equal(p1.view(np.uint32), got.view(np.uint32)):
                    break
            else:
                p1, _ = oc.param_f32(p, m, v, cands[0][1], cands[0][2])
                d = p1.view(np.uint32) != got.view(np.uint32)
                raise AssertionError(f"{w}: t = {t}: {'the reference scalars do' if exact else 'none of the nine scalar pairs does'} "
                                     f"not give the parameters; with the reference pair {d.sum()} of {n} differ, first at "
                                     f"{int(d.argmax())}: got {got[d.argmax()]!r}, want {p1[d.argmax()]!r}")
            p, p16 = p1, p16_1
            matched.append((t, label))
            stepped_p.append(got)
            if train:
                q, sm, sv = oc.small_step(q, sm, sv, oc.small_grads(k), inv_small, lr, *run.betas, t, scalars=(s, b))
        invs.append(inv)
        for name, want in (("p", p), ("m", m), ("v", v), ("p16", p16)):
            _same(snap[name], want, f"{w} {name}")
        if train:
            for i, want in enumerate(q):
                _same(snap[f"q{i}"], want, f"{w} small tensor {i}")
            _same(snap["sm"], sm, w + " small exp_avg")
            _same(snap["sv"], sv, w + " small exp_avg_sq")
        else:
            assert _host(snap["t"], 1)[0] == float(t) and bool((snap["t"][1:] == SENT).all()), w + ": step counter"
    ratio, mult = oc.tier_b_ratio(stepped_p, run, invs)
    print(f"{what}: scalar pairs {matched}; tier B: |p - p64| / bound {ratio:.3f}, largest multiple of 2^-24 A {mult:.2f} "
          f"(K {oc.k_of_step(1)} .. {oc.k_of_step(t)})")
    assert ratio <= 1.0, f"{what}: |p - p64| is {ratio:.2f} times the derived bound"
    return matched


# ================================================================================================ tier A and B: the table runs
@pytest.mark.parametrize("entry", ["adam", "train_step"])
@pytest.mark.parametrize("name", oc.RUN_NAMES)
def test_run_bit_for_bit_and_within_the_float64_bound(name, entry):
    run = oc.get_run(name)
    a, b = execute(run, entry), execute(run, entry)
    for k, (x, y) in enumerate(zip(a, b)):
        _equal_snaps(x, y, f"{name} [{entry}] call {k}: two identical runs")
    verify(run, entry, a)


@pytest.mark.parametrize("name", ["big_three_calls", "n1027_exact_betas", "n3_first_1/3072"])
def test_dlr_is_the_same_step_bit_for_bit(name):
    run = oc.get_run(name)
    a, b = execute(run, "adam"), execute(run, "dlr")
    for k, (x, y) in enumerate(zip(a, b)):
        _equal_snaps(x, y, f"{name} call {k}: lnh_adam_table_step_dlr against lnh_adam_table_step")
    assert _host(a[-1]["t"], 1)[0] == sum(run.steps)


def test_null_gradient_tensors_keep_their_moments_and_offsets_hold():
    """One step of the sixteen small tensors alone (n = 0): every tensor's moments lie at the sum of the sizes before it — the
    moments start at a value of their own per tensor — and those of the three tensors without a gradient keep every bit."""
    rig = Rig(4)
    G, SG, gp = rig.grads(0)
    before = rig.snap()
    rig.check(None, 0, gp)
    rig.step(None, gp, table=False)
    after = rig.snap()
    a = oc.train_check(oc.new_state(IT_NEXT=oc.ITERS), False, 1.0, oc.DIV_SMALL, oc.LR0, oc.ITERS)
    ps, ms, vs = oc.small_inputs()
    q, sm, sv = oc.small_step(ps, np.concatenate(ms), np.concatenate(vs), oc.small_grads(0), a[oc.INV], float(a[oc.LR]),
                              *oc.PROD_BETAS, 1)
    offs = oc.small_offsets()
    for k in oc.SMALL_NULL:
        sl = slice(offs[k], offs[k] + oc.SMALL_NUMEL[k])
        assert np.array_equal(sm[sl], ms[k]) and np.array_equal(sv[sl], vs[k]) and np.array_equal(q[k], ps[k])
    for i, want in enumerate(q):
        _same(after[f"q{i}"], want, f"small tensor {i}")
    _same(after["sm"], sm, "small exp_avg")
    _same(after["sv"], sv, "small exp_avg_sq")
    _same(after["state"], oc.train_step(a)[0], "state")
    for k in ("p", "m", "v", "p16"):
        assert torch.equal(_ibits(before[k]), _ibits(after[k])), f"n = 0 touched the table's {k}"


# ================================================================================================ the finite check
def _i16(pattern):
    return int(np.array(pattern, np.uint16).view(np.int16))


@pytest.mark.parametrize("entry", ["lnh_grad_check_f16", "lnh_train_check"])
@pytest.mark.parametrize("pattern", list(oc.BAD_PATTERNS))
def test_one_bad_value_anywhere_is_found(pattern, entry):
    """One inf / nan per call at every position of check_positions(); a clean buffer of +-65504, subnormals and +-0 of every
    length sets nothing; the words behind n are NaN and are never taken for gradient values."""
    fill = oc.finite_fill16(oc.CHECK_BASE + 7)
    G = _grad16(fill)
    Gi, fill_d = G.view(torch.int16), _up(fill.view(np.int16))
    st0 = oc.new_state(IT_NEXT=6.0, FOUND=3.0)
    gp = _H().ptr_array([None])
    nn = _H().u32_array([0])

    def found(n):
        if entry == "lnh_grad_check_f16":
            f = _io(np.zeros(1, F32))
            _call(entry, G, n, f.buf)
            got = _host(f.buf, 1 + GUARD)
            assert (got[1:] == SENT).all() and got[0] in (0.0, 1.0)
            return got[0] == 1.0
        st = _io(st0)
        _call(entry, st.buf, G, n, _cast(gp), _cast(nn), 0, 1.0, 1.0, oc.LR0, oc.ITERS)
        bad = _host(st.buf, oc.STATE_FLOATS)[oc.FOUND] != 3.0
        _same(st.buf, oc.train_check(st0, bad, 1.0, 1.0, oc.LR0, oc.ITERS), f"{entry} state, n = {n}")   # the stamp is 7
        return bad

    last_n = None
    for n, i in oc.check_positions():
        if n != last_n:
            Gi[oc.CHECK_BASE:n] = fill_d[oc.CHECK_BASE:n]
            Gi[n:oc.CHECK_BASE + 7] = _i16(0x7e00)
            assert not found(n), f"{entry}: a finite buffer of n = {n} was reported"
            last_n = n
        Gi[i] = _i16(oc.BAD_PATTERNS[pattern])
        hit = found(n)
        Gi[i] = int(fill_d[i])
        assert hit, f"{entry}: {pattern} at index {i} of n = {n} (lane {i % 8}) was not found"


def test_grad_check_never_clears_and_takes_n_zero():
    G = _grad16(oc.finite_fill16(4099))
    for preset in (1.0, 5.0):
        f = _io(np.full(1, preset, F32))
        _call("lnh_grad_check_f16", G, 4099, f.buf)
        _call("lnh_grad_check_f16", G, 0, f.buf)
        _same(f.buf, np.full(1, preset, F32), "found_inf after clean gradients")
    G.view(torch.int16)[4098] = _i16(0xfc00)
    f = _io(np.full(1, 5.0, F32))
    _call("lnh_grad_check_f16", G, 4098, f.buf)      # the inf lies behind n
    _same(f.buf, np.full(1, 5.0, F32), "found_inf")
    _call("lnh_grad_check_f16", G, 4099, f.buf)
    _same(f.buf, np.full(1, 1.0, F32), "found_inf")


@pytest.mark.parametrize("n16", [0, 1027])
def test_small_gradients_are_checked_everywhere(n16):
    """fp32 gradients of +-FLT_MAX, subnormals and +-0 set nothing; one inf / nan at the first, the last and the first strided
    elements of the largest tensor, in a one-element tensor and in the tensors behind those without a gradient is stamped.
    n16 = 0 passes a null table gradient (one workgroup: stride 256); n16 = 1027 has two workgroups (stride 512)."""
    H = _H()
    nn = H.u32_array(oc.SMALL_NUMEL)
    G = _grad16(oc.finite_fill16(n16)) if n16 else None
    host = [None if k in oc.SMALL_NULL else oc.finite_fill32(n, 20 + k).view(F32) for k, n in enumerate(oc.SMALL_NUMEL)]
    SG = [None if g is None else _grad32(g) for g in host]
    gp = H.ptr_array([None if g is None else g.data_ptr() for g in SG])
    st0 = oc.new_state(IT_NEXT=2.0)

    def stamped():
        st = _io(st0)
        _call("lnh_train_check", st.buf, G, n16, _cast(gp), _cast(nn), 16, 2.0, 4.0, oc.LR0, 100.0)
        got = _host(st.buf, oc.STATE_FLOATS)
        want = oc.train_check(st0, got[oc.FOUND] != 0.0, 2.0, 4.0, oc.LR0, 100.0)
        lr_ulps = abs(int(got[oc.LR:oc.LR + 1].view(np.int32)[0]) - int(want[oc.LR:oc.LR + 1].view(np.int32)[0]))
        assert lr_ulps <= 1, "LR inside the schedule is more than one ulp off"
        want[oc.LR] = got[oc.LR]
        _same(st.buf, want, "state")
        return got[oc.FOUND] == 3.0

    assert not stamped(), "finite small gradients were reported"
    where = [(7, 0), (7, 256), (7, 512), (7, 16384), (7, 16640), (1, 0), (10, 3), (14, 512), (15, 32), (5, 16383), (6, 16384)]
    for j, (k, i) in enumerate(where):
        assert k not in oc.SMALL_NULL and i < oc.SMALL_NUMEL[k]
        for name, pat in list(oc.BAD_PATTERNS32.items())[j % 2::2] if j > 4 else oc.BAD_PATTERNS32.items():
            view = SG[k].view(torch.int32)
            keep = int(view[i])
            view[i] = int(np.array(pat, np.uint32).view(np.int32))
            hit = stamped()
            view[i] = keep
            assert hit, f"{name} at element {i} of small gradient {k} was not found"
    assert not stamped()


# ================================================================================================ bookkeeping
@pytest.mark.parametrize("name", [s.name for s in oc.SCENARIOS])
def test_bookkeeping_scenario(name):
    """`state` as integers after every call of a scripted run; a skipped step leaves every byte of every buffer alone."""
    sc = next(s for s in oc.SCENARIOS if s.name == name)
    st = oc.new_state()
    for k, val in sc.init.items():
        st[oc.SLOT_NAMES.index(k)] = val
    rig = Rig(1027, 1, st)
    t0 = float(st[oc.T_NEXT])
    any_skip = False
    for k, ((bad, preset), (a, b, skip)) in enumerate(zip(sc.steps, oc.run_scenario(sc))):
        w = f"{name} step {k}"
        if preset is not None:
            rig.st.data()[oc.FOUND] = float(a[oc.IT]) + preset
        G, SG, gp = rig.grads(k % 7, (("table", "small")[k % 2]) if bad else None)
        before = rig.snap()
        rig.check(G, rig.n, gp, div_table=sc.div_table, div_small=sc.div_small, lr0=sc.lr0, iters=sc.iters)
        got = _host(rig.st.buf, oc.STATE_FLOATS)
        if not oc.lr_is_exact(float(a[oc.IT]), sc.iters):
            ulps = abs(int(got[oc.LR:oc.LR + 1].view(np.int32)[0]) - int(a[oc.LR:oc.LR + 1].view(np.int32)[0]))
            assert ulps <= 1, f"{w}: LR {got[oc.LR]!r} against {a[oc.LR]!r}"
            a, b = a.copy(), b.copy()
            a[oc.LR] = b[oc.LR] = got[oc.LR]
        _same(rig.st.buf, a, w + " state after the check")
        rig.step(G, gp, interval=sc.interval)
        after = rig.snap()
        _same(after["state"], b, w + " state after the step")
        assert float(b[oc.SKIPPED]) == float(skip)
        moved = [key for key in before if key != "state" and not torch.equal(_ibits(before[key]), _ibits(after[key]))]
        if skip:
            any_skip = True
            assert not moved, f"{w}: a skipped step wrote {moved}"
        else:
            assert {"m", "sm", "p16"} <= set(moved) or (k > 0 and {"m", "sm"} <= set(moved)), f"{w}: a step that was not skipped left buffers alone"
    assert any_skip == any(s for _, _, s in oc.run_scenario(sc))
    assert float(_host(rig.st.buf, 16)[oc.T_NEXT]) == t0 + sum(not s for _, _, s in oc.run_scenario(sc))


@pytest.mark.parametrize("bad", [True, False])
def test_check_in_three_pieces(bad):
    """lnh_train_check once per piece [0, a), [a, b), [b, n) of the table gradient, the small gradients with the first: the
    committed values keep their bits from call to call; an inf in the second piece skips the step; without one the step is the
    step of a one-call check."""
    n, a, b = 1027, 256, 768
    whole, rig = Rig(n), Rig(n)
    G, SG, gp = rig.grads(0, "table" if bad else None)
    assert a <= n // 2 < b and a % 8 == 0 and b % 8 == 0
    whole.check(G, n, gp, div_table=3.0)
    kept = None
    for k, (lo, hi) in enumerate(((0, a), (a, b), (b, n))):
        rig.check(G.data_ptr() + 2 * lo, hi - lo, gp, n_small=16 if k == 0 else 0, div_table=3.0)
        got = _host(rig.st.buf, oc.STATE_FLOATS)
        assert got[oc.FOUND] == (oc.ITERS + 1.0 if bad and k >= 1 else 0.0), f"piece {k}: FOUND = {got[oc.FOUND]}"
        slots = got[[oc.T, oc.IT, oc.INV, oc.INV_TABLE, oc.LAST_SCALE, oc.LR]].view(np.int32)
        assert kept is None or np.array_equal(kept, slots), f"piece {k} changed a committed value"
        kept = slots
    assert torch.equal(_ibits(rig.st.buf), _ibits(whole.st.buf))
    before = rig.snap()
    whole.step(G, gp)
    rig.step(G, gp)
    _equal_snaps(whole.snap(), rig.snap(), "three pieces against one call")
    after = rig.snap()
    assert _host(after["state"], 16)[oc.SKIPPED] == float(bad)
    moved = [k for k in before if k != "state" and not torch.equal(_ibits(before[k]), _ibits(after[k]))]
    assert (not moved) if bad else {"p", "m", "v", "p16", "sm", "sv"} <= set(moved)


def test_sharded_wiring_equals_one_whole_step():
    """lnh_train_step(n = 0, small tensors) and lnh_adam_table_step_dlr per slice on the state's LR, INV_TABLE, SKIPPED, T and
    T_NEXT (the sharded trainer's calls) against one lnh_train_step: four steps, the third one bad."""
    n, cuts = 1027, (0, 256, 640, 640, 1027)
    whole, rig = Rig(n), Rig(n)
    sp = lambda i: rig.st.buf.data_ptr() + 4 * i
    for k in range(4):
        G, SG, gp = rig.grads(k, "small" if k == 2 else None)
        for r in (whole, rig):
            r.check(G, n, gp, div_table=3.0)
        whole.step(G, gp)
        rig.step(None, gp, table=False)
        for lo, hi in zip(cuts, cuts[1:]):
            if hi > lo:
                assert lo % 4 == 0
                _call("lnh_adam_table_step_dlr", rig.P.buf.data_ptr() + 4 * lo, rig.M.buf.data_ptr() + 4 * lo,
                      rig.V.buf.data_ptr() + 4 * lo, G.data_ptr() + 2 * lo, rig.P16.buf.data_ptr() + 2 * lo, hi - lo, sp(oc.LR),
                      *oc.PROD_BETAS, EPS, sp(oc.INV_TABLE), sp(oc.SKIPPED), sp(oc.T), sp(oc.T_NEXT))
        _equal_snaps(whole.snap(), rig.snap(), f"step {k}: shards against the whole step")
        st = _host(rig.st.buf, 16)
        assert st[oc.SKIPPED] == float(k == 2) and st[oc.T_NEXT] == k + 1 - (k >= 2)
        assert bool((rig.st.buf[16:] == SENT).all())


# ================================================================================================ lnh_zero_regions
def _regions(spec):
    """Per region: a float32 buffer of 7.0 with 8 guard words on both sides; the region starts `offset` bytes past a 16-byte
    boundary.  -> [(buffer, first word, words)]"""
    out = []
    for r in spec:
        if r is None:
            out.append(None)
            continue
        off, nbytes = r
        first, words = 8 + off // 4, nbytes // 4
        buf = torch.full((first + words + 8,), 7.0, device="cuda")
        assert (buf.data_ptr() + 4 * first) % 16 == off
        out.append((buf, first, words))
    return out


def _zero(regs, ptr_shift=0, size_shift=0):
    ptrs = (C.c_void_p * max(len(regs), 1))(*[None if r is None else r[0].data_ptr() + 4 * r[1] + ptr_shift for r in regs])
    sizes = (C.c_uint64 * max(len(regs), 1))(*[0 if r is None else 4 * r[2] + (size_shift if r[2] else 0) for r in regs])
    _call("lnh_zero_regions", _cast(ptrs), _cast(sizes), len(regs))


@pytest.mark.parametrize("spec", [oc.ZERO_CALL_1, oc.ZERO_CALL_2], ids=["with_the_big_region", "short_regions"])
def test_zero_regions_clears_exactly_the_regions(spec):
    regs = _regions(spec)
    _zero(regs)
    for i, r in enumerate(regs):
        if r is None:
            continue
        buf, first, words = r
        inside = buf[first:first + words].view(torch.int32)
        assert bool((inside == 0).all()), f"region {i} {spec[i]}: {int((inside != 0).sum())} words were not cleared"
        assert bool((buf[:first] == 7.0).all()) and bool((buf[first + words:] == 7.0).all()), f"region {i} {spec[i]}: a guard word was cleared"


def test_zero_regions_refusals_leave_the_buffers_alone():
    nine = _regions(((0, 16),) * 9)
    eight = _regions(((0, 16),) * 8)
    for regs, kw in ((nine, {}), (eight, {"size_shift": 2}), (eight, {"ptr_shift": 2})):
        with pytest.raises(RuntimeError):
            _zero(regs, **kw)
        torch.cuda.synchronize()
        assert all(bool((r[0] == 7.0).all()) for r in regs)
    _zero([])   # no region: accepted


# ================================================================================================ refusals
def test_refusals_launch_nothing():
    H = _H()
    rig = Rig(1027)
    G, SG, gp = rig.grads(0)
    rig.check(G, rig.n, gp)       # a valid check first: the refused calls see a state a step could run on
    found, inv, lr = _io(np.zeros(1, F32)), _up(np.array([2.0 ** -10], F32)), _up(np.array([oc.RUN_LR], F32))
    s_in, s_out = _io(np.zeros(1, F32)), _io(np.zeros(1, F32))
    before = dict(rig.snap(), found=found.buf.clone(), s_in=s_in.buf.clone(), s_out=s_out.buf.clone())
    pp17, gp17, nn17 = H.ptr_array([rig.Q[1].buf.data_ptr()] * 17), H.ptr_array([SG[1].data_ptr()] * 17), H.u32_array([1] * 17)
    P, M, V, P16, st = rig.P.buf, rig.M.buf, rig.V.buf, rig.P16.buf, rig.st.buf
    adam = lambda p=P, g=G, si=s_in.buf, so=s_out.buf: _call(
        "lnh_adam_table_step", p, M, V, g, P16, rig.n, oc.RUN_LR, *oc.PROD_BETAS, EPS, inv, found.buf, si, so)
    dlr = lambda lrp=lr, si=s_in.buf, so=s_out.buf: _call(
        "lnh_adam_table_step_dlr", P, M, V, G, P16, rig.n, lrp, *oc.PROD_BETAS, EPS, inv, found.buf, si, so)
    check = lambda s=st, g=G, ns=16, g_p=gp, n_p=rig.nn, dt=1.0, ds=1.0, iters=oc.ITERS: _call(
        "lnh_train_check", s, g, rig.n, _cast(g_p), _cast(n_p), ns, dt, ds, oc.LR0, iters)
    step = lambda s=st, p=P, g=G, ns=16, p_p=rig.pp, g_p=gp, n_p=rig.nn, sm=rig.SM.buf, sv=rig.SV.buf: _call(
        "lnh_train_step", s, p, M, V, g, P16, rig.n, _cast(p_p), _cast(g_p), _cast(n_p), ns, sm, sv, *oc.PROD_BETAS, EPS, *SCALING, 2000)
    refused = {
        "check: 17 small tensors": lambda: check(ns=17, g_p=gp17, n_p=nn17),
        "step: 17 small tensors": lambda: step(ns=17, p_p=pp17, g_p=gp17, n_p=nn17),
        "adam: param offset by 4 bytes": lambda: adam(p=P.data_ptr() + 4),
        "step: param offset by 4 bytes": lambda: step(p=P.data_ptr() + 4),
        "grad_check: grad16 offset by 2 bytes": lambda: _call("lnh_grad_check_f16", G.data_ptr() + 2, 1000, found.buf),
        "check: grad16 offset by 2 bytes": lambda: check(g=G.data_ptr() + 2),
        "adam: grad16 offset by 2 bytes": lambda: adam(g=G.data_ptr() + 2),
        "step: grad16 offset by 2 bytes": lambda: step(g=G.data_ptr() + 2),
        "adam: step_in == step_out": lambda: adam(si=s_in.buf, so=s_in.buf),
        "dlr: step_in == step_out": lambda: dlr(si=s_in.buf, so=s_in.buf),
        "dlr: null lr": lambda: dlr(lrp=None),
        "check: div_table = 0": lambda: check(dt=0.0),
        "check: div_small = 0": lambda: check(ds=0.0),
        "check: iters = 0": lambda: check(iters=0.0),
        "step: null exp_avg of the small tensors": lambda: step(sm=None),
        "step: null exp_avg_sq of the small tensors": lambda: step(sv=None),
        "check: null state": lambda: check(s=None),
        "step: null state": lambda: step(s=None),
        "grad_check: null found_inf": lambda: _call("lnh_grad_check_f16", G, 1000, None),
    }
    for what, fn in refused.items():
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"{what}: accepted")
        torch.cuda.synchronize()
        after = dict(rig.snap(), found=found.buf.clone(), s_in=s_in.buf.clone(), s_out=s_out.buf.clone())
        _equal_snaps(before, after, what)
    step()   # the state is still one a step runs on
    assert _host(rig.st.buf, 16)[oc.T_NEXT] == 1.0
