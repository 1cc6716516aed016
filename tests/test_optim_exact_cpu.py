"""The problems of tests/test_optim_exact_gpu.py checked without a GPU (tests/optim_exact_cases.py): the float64 reference is
torch.optim.Adam in float64, the float32 restatement lies within the tier B bound of it, the scale rule is torch's
_amp_update_scale_ (this torch build offers it on CPU tensors, so it is compared directly, not against a table), the sizes and
positions cover what they promise, and every named mistake changes an expected value — the arithmetic ones beyond the bound."""
import fractions
import math

import numpy as np
import pytest
import torch

import optim_exact_cases as oc

F32 = np.float32
SMALL_RUNS = [n for n in oc.RUN_NAMES if oc.get_run(n).n <= 20000]


def _stepped(ref, run):
    return [r[0] for r, s in zip(ref, run.steps) if s]


@pytest.mark.parametrize("name", SMALL_RUNS)
def test_float64_reference_is_torch_adam_in_float64(name):
    run = oc.get_run(name)
    p0, grads = oc.run_inputs(run)
    ref = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([ref], lr=run.lr, betas=run.betas, eps=oc.EPS, fused=False, foreach=False)
    want = iter(oc.run_reference64(run))
    for g, stepped in zip(grads, run.steps):
        if not stepped:
            continue
        ref.grad = torch.from_numpy(g.view(np.float16).astype(np.float64) * float(oc.INVS[run.inv]))
        opt.step()
        st, _ = next(want)
        so = opt.state[ref]
        assert np.abs(ref.detach().numpy() - st.p).max() <= 1e-12 * np.abs(st.A).max()
        assert (np.abs(ref.detach().numpy() - st.p) <= 1e-12 * st.A).all()
        assert (np.abs(so["exp_avg"].numpy() - st.m) <= 1e-14 * st.am).all()
        assert (np.abs(so["exp_avg_sq"].numpy() - st.v) <= 1e-14 * st.v).all()
        assert (st.am >= np.abs(st.m) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", SMALL_RUNS)
def test_restatement_lies_within_the_bound_of_tier_b(name):
    run = oc.get_run(name)
    ratio, mult = oc.tier_b_ratio(_stepped(oc.run_reference(run), run), run)
    print(f"{name}: |p - p64| / bound {ratio:.3f}, largest multiple of 2^-24 A {mult:.2f} (K {oc.k_of_step(1)} .. {oc.k_of_step(6)})")
    assert ratio <= 1.0


def test_k_is_the_count_of_its_docstring():
    assert [oc.k_of_step(s) for s in range(1, 7)] == [13, 14, 16, 17, 19, 20]
    assert all(oc.k_of_step(s) >= 1.5 * s + 11 for s in range(1, 40))


@pytest.mark.parametrize("mistake", oc.ARITHMETIC)
def test_arithmetic_mistakes_break_the_bound_of_tier_b(mistake):
    """A mistake copied from the kernel into the float32 restatement would fail tier B: every arithmetic one does, on every
    six-step run."""
    for name in oc.SIX_STEP_RUNS:
        run = oc.get_run(name)
        ratio, _ = oc.tier_b_ratio(_stepped(oc.run_reference(run, mistake=mistake), run), run)
        assert ratio > 1.0, (mistake, name, ratio)


def test_scale_rule_is_torchs_amp_update_scale():
    if not hasattr(torch, "_amp_update_scale_"):
        pytest.fail("this torch build has no _amp_update_scale_: pin the rule to a literal table instead")
    for scale in (1024.0, 2.0 ** 127, 2.0 ** -10, 65536.0, 1.0):
        for interval in (1, 2, 3, 2000):
            for tracker in sorted({0, 1, interval - 2, interval - 1} - {-1}):
                for found in (0.0, 1.0):
                    s, g = torch.tensor(scale), torch.tensor(tracker, dtype=torch.int32)
                    torch._amp_update_scale_(s, g, torch.tensor(found), 2.0, 0.5, interval)
                    got = oc.amp_update_scale(scale, float(tracker), found, 2.0, 0.5, interval)
                    assert got == (float(s), float(g)), (scale, interval, tracker, found, got)
    assert oc.amp_update_scale(2.0 ** 127, 2.0, False, interval=3) == (2.0 ** 127, 0.0)       # held, the counter reset
    assert oc.amp_update_scale(1024.0, 2.0, True, interval=3) == (512.0, 0.0)                 # back-off wins over growth


def test_finite_predicate_is_isfinite():
    b16 = np.arange(65536, dtype=np.uint16)
    assert np.array_equal((b16 & 0x7c00) == 0x7c00, ~np.isfinite(b16.view(np.float16)))
    rng = np.random.default_rng(0)
    b32 = np.concatenate([rng.integers(0, 2 ** 32, 100000).astype(np.uint32), np.array(list(oc.BAD_PATTERNS32.values()), np.uint32),
                          oc.finite_fill32(100)])
    assert np.array_equal((b32 & 0x7f800000) == 0x7f800000, ~np.isfinite(b32.view(np.float32)))
    assert all(oc.bad16([b]) for b in oc.BAD_PATTERNS.values()) and all(oc.bad32([b]) for b in oc.BAD_PATTERNS32.values())
    assert not oc.bad16(oc.finite_fill16(4096)) and not oc.bad32(oc.finite_fill32(4096))
    assert {0x7bff, 0xfbff, 0x0001, 0x8000} <= set(oc.finite_fill16(4096).tolist())
    assert {0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000000} <= set(oc.finite_fill32(4096).tolist())


def test_sizes_and_positions_cover_what_they_promise():
    bc = oc.block_count
    # both grid-stride caps are passed, with a tail behind the second trip
    assert oc.N_BIG > oc.TRIP and oc.N_BIG > oc.CHECK_TRIP and oc.N_BIG % 4 == 3 and oc.N_BIG // 4 > oc.TABLE_WG_CAP * oc.WG
    assert oc.TRIP == oc.CHECK_TRIP == 4194304
    # the block formula switches between the first two boundary sizes; the third is the last size without a second trip
    a, b, c = oc.N_BOUNDARY
    assert (bc(a, 4, 4096), bc(b, 4, 4096), bc(c, 4, 4096)) == (4096, 4096, 4096)
    assert (a // 4 + 255) // 256 == 4095 and (b // 4 + 255) // 256 == 4096 and bc(a - 4 * 256, 4, 4096) == 4095
    assert c == oc.TRIP and bc(oc.N_BIG, 4, 4096) == 4096
    assert {r.n for r in oc.RUNS} >= set(oc.N_SMALL_SHAPES) | set(oc.N_BOUNDARY) | {oc.N_BIG}
    assert any(not all(r.steps) for r in oc.RUNS if r.n == oc.N_BIG) and len(oc.get_run("big_three_calls").steps) == 3
    assert {r.inv for r in oc.RUNS if r.n in oc.N_SMALL_SHAPES and r.betas == oc.PROD_BETAS} == set(oc.INVS)
    assert float(oc.INVS["1/3072"]) not in (2.0 ** -k for k in range(40))
    # bad-value positions: all 8 lanes of a vector, both trips, the last whole vector, every tail length and position
    pos = oc.check_positions()
    whole = [i for n, i in pos if n == oc.CHECK_BASE]
    assert {i % 8 for i in whole if i < 8} == set(range(8))
    assert {i % 8 for i in whole if oc.CHECK_TRIP - 8 <= i < oc.CHECK_TRIP} == set(range(8))
    assert {i % 8 for i in whole if oc.CHECK_TRIP <= i < oc.CHECK_TRIP + 8} == set(range(8))
    assert {i for i in whole if i >= oc.CHECK_BASE - 8} == set(range(oc.CHECK_BASE - 8, oc.CHECK_BASE))
    assert {(n - oc.CHECK_BASE, i - oc.CHECK_BASE) for n, i in pos if n > oc.CHECK_BASE} == {(t, j) for t in range(1, 8) for j in range(t)}
    assert oc.CHECK_BASE % 8 == 0 and bc(oc.CHECK_BASE, 8, 2048) == 2048 and oc.CHECK_BASE > oc.CHECK_TRIP
    # small tensors: sixteen, one empty, three without a gradient (one of them the empty one), sizes around one block and one trip
    assert len(oc.SMALL_NUMEL) == oc.MAX_SMALL == 16 and oc.SMALL_NUMEL[0] == 0 and 0 in oc.SMALL_NULL and len(oc.SMALL_NULL) == 3
    assert {0, 1, 255, 256, 257, 16384, 16385, 16641} <= set(oc.SMALL_NUMEL) and oc.SMALL_TRIP == 16384 and oc.SMALL_BLOCKS == 64
    assert any(oc.SMALL_NUMEL[k] > 0 and k + 1 < 16 for k in oc.SMALL_NULL)
    # zero regions: every head alignment, lengths below / at / past the head, the workgroup cap of a region
    for call in (oc.ZERO_CALL_1, oc.ZERO_CALL_2):
        assert len(call) == 8
    regs = [r for r in oc.ZERO_CALL_1 + oc.ZERO_CALL_2 if r]
    assert {o for o, _ in regs} == {0, 4, 8, 12} and {4, 8, 12, 16, 20, 44, 0} <= {b for _, b in regs}
    head = lambda o: (16 - o) % 16
    assert any(b < head(o) for o, b in regs if b) and any(b == head(o) for o, b in regs if b) and any(b == head(o) + 4 for o, b in regs)
    assert (oc.ZERO_BIG_BYTES // 16 + 1023) // 1024 > oc.ZERO_WG_CAP and None in oc.ZERO_CALL_1 and (12, 0) in oc.ZERO_CALL_1


def test_inputs_reach_the_edges():
    p, z = oc.table_params(), oc.zero_mask()
    assert np.abs(p).max() <= 1e-4 and (np.abs(p) < 2.0 ** -14).mean() > 0.3            # fp16 subnormals in p16
    ties = p[z].astype(np.float64) * 2.0 ** 25
    assert (ties == np.round(ties)).all() and (np.round(ties) % 2 == 1).all()           # odd multiples of 2^-25: fp16 ties
    assert (np.abs(p[z]) < 2.0 ** -14).any() and (np.abs(p[z]) > 2.0 ** -14).any()
    for step in range(3):
        g = oc.table_grad(step)
        assert not oc.bad16(g) and z.mean() > 0.14 and (g[z] & 0x7fff == 0).all() and {0, 0x8000} <= set(g[z][:8].tolist())
        assert tuple(g[1:7]) == oc.SPECIALS and ((g & 0x7fff) < 0x0400).mean() > 0.02   # the extremes, plenty of subnormals
        assert len(np.unique(g >> 10 & 0x1f)) == 31                                     # every finite exponent
    # exp_avg_sq stays far above the float32 subnormals (2^-126), zero where the gradient is always zero
    for name in ("big_three_calls",) + oc.SIX_STEP_RUNS:
        run = oc.get_run(name)
        zz = z[run.off:run.off + run.n]
        for r in oc.run_reference(run):
            v, m = r[2], r[1]
            assert (v[zz] == 0).all() and (m[zz] == 0).all() and v[v > 0].min() > 2.0 ** -100 and (v[~zz] > 0).mean() > 0.99
            assert np.array_equal(r[0][zz].view(np.uint32), p[run.off:run.off + run.n][zz].view(np.uint32))   # p stays put to the bit


def test_exact_betas_have_exact_powers():
    for b in oc.EXACT_BETAS:
        for t in range(1, 5):
            assert fractions.Fraction(b) ** t == fractions.Fraction(b ** t) == fractions.Fraction(float(np.float64(b) ** t))
    for t in range(2, 7):   # the nine candidates are distinct floats around the centre
        c = oc.candidates(oc.RUN_LR, *oc.PROD_BETAS, t)
        assert len({(float(s), float(b)) for _, s, b in c}) == 9 and c[0][0] == (0, 0)


def test_learning_rate_is_exact_at_both_ends_of_the_schedule():
    sc = oc.SCENARIOS[0]
    states = [a for a, _, _ in oc.run_scenario(sc)]
    assert [float(a[oc.IT]) for a in states] == list(range(10))
    assert float(states[0][oc.LR]) == sc.lr0 and all(a[oc.LR] == F32(sc.lr0 * 0.1) for a in states[4:])
    assert [oc.lr_is_exact(i, sc.iters) for i in range(6)] == [True, False, False, False, True, True]
    assert F32(sc.lr0) == sc.lr0 and math.frexp(sc.lr0)[0] == 0.5
    # the runs: they start at IT = ITERS, their LR and their 1 / scale are what the state machine forms
    for name, (scale, div) in oc.INV_SOURCE.items():
        a = oc.train_check(oc.new_state(scale, IT_NEXT=oc.ITERS), False, div, oc.DIV_SMALL, oc.LR0, oc.ITERS)
        assert a[oc.INV_TABLE] == oc.INVS[name] and float(a[oc.LR]) == oc.RUN_LR and a[oc.INV] == F32(1.0) / F32(scale) / F32(4.0)
    assert all(r.lr == oc.RUN_LR for r in oc.RUNS)


WALK = ("tail_off_by_one", "second_trip_stride_griddim")


def _expectations(mistake, big):
    """Everything the GPU file compares, as a flat list of arrays, under a mistake (`big`: with the N_BIG run)."""
    out = []
    for run in oc.RUNS:
        if run.n > 20000 and not (big and run.name == "big_three_calls"):
            continue
        for entry in ("adam", "train_step"):
            for r in oc.run_reference(run, entry, oc.SMALL_BLOCKS if entry == "train_step" else 0, mistake):
                out += [r[0], r[1], r[2], r[3].view(np.uint16)]
    ps, ms, vs = oc.small_inputs()
    sm, sv = np.concatenate(ms), np.concatenate(vs)
    q, sm, sv = oc.small_step(ps, sm, sv, oc.small_grads(0), F32(2.0 ** -12), 2.0 ** -6, *oc.PROD_BETAS, 1, mistake)
    out += q + [sm, sv]
    for sc in oc.SCENARIOS:
        for a, b, _ in oc.run_scenario(sc, mistake):
            out += [a, b]
    for tl in range(8):          # one bad value at every position of a whole vector and of every tail behind one
        for i in list(range(8)) + [8 + j for j in range(tl)]:
            buf = oc.finite_fill16(8 + tl)
            buf[i] = 0x7c00
            out.append(np.array([oc.bad16(buf, mistake=mistake)]))
    return out


@pytest.mark.parametrize("mistake", oc.MISTAKES)
def test_every_mistake_changes_an_expected_value(mistake):
    right, wrong = _expectations(None, mistake in WALK), _expectations(mistake, mistake in WALK)
    assert len(right) == len(wrong)
    assert any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(right, wrong)), mistake
