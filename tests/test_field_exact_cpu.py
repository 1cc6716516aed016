"""The exact LiDAR-field problems of tests/test_field_exact_gpu.py, checked without a GPU: every shape that file uses must meet
the conditions that make a bit-for-bit comparison meaningful (tests/field_exact_cases.py: 16-bit exactness, the 2^24 sum bound,
live and distinct units, a probe in every position class, compensated gradients that survive a perturbed sigmoid in fp16 and in
bf16) and must tell the classic kernel mistakes apart from the right answer; problems that break a condition must be rejected."""
import numpy as np
import pytest

import field_exact_cases as fc

DENSE = fc.COLOR_FWD_SHAPES + fc.COLOR_BWD_SHAPES + fc.COLOR_WAVE_SHAPES


@pytest.mark.parametrize("shape", fc.SIGMA_SHAPES + [fc.SIGMA_FWD_STRIDE, fc.SIGMA_BWD_STRIDE])
def test_sigma_net_problems(shape):
    s = fc.get_sigma_case(*shape)  # (asserts its conditions; the MLP problem under it asserted its own in get_case)
    fc.mc.check_discrimination(s.c)
    assert s.B == shape[0] * shape[1] and s.rows[0] == shape[3] and s.rows[-1] == s.B_all - (shape[2] - shape[1] - shape[3]) - 1
    N, Tc, Tt, off = fc.SIGMA_FWD_STRIDE
    assert N * Tc > 2048 * 128 and fc.get_sigma_case(N, Tc, Tt, off).c.P == fc.mc.PERIOD
    N, Tc, Tt, off = fc.SIGMA_BWD_STRIDE
    assert N * Tc > 256 * 256


@pytest.mark.parametrize("N,T", DENSE)
def test_colour_head_problems(N, T):
    c = fc.get_color_case(N, T)  # (asserts check_conditions)
    fc.check_discrimination(c)
    e = c.expected()
    for k in ("dW0g", "dW1", "dW2", "S"):
        assert np.array_equal(e[k], np.rint(e[k])) and np.abs(e[k]).max() < fc.SUM_LIMIT
    assert not np.any(e["dW2"][2:]) and np.all(e["g_h16"][:, 0] != 0)
    masked = ~c.act
    assert not np.any(e["rgb"][c.pos[masked]]) and np.all(e["rgb"][c.pos[c.act]] > 0)


def test_position_classes_are_all_met_somewhere():
    """Every position class of the backward's span iterator is held by some problem: spans and groups in the small shapes, the pipeline and multi-ray patterns in the shapes with more
    rays than resident waves; the larger problems carry the unit conditions (>= 200 probes)."""
    met = set()
    for N, T in DENSE:
        c = fc.get_color_case(N, T)
        met |= {k for k, v in c.position_classes().items() if v and k in fc.required_classes(c)}
    assert met == {"last valid sample of a partial span", "first sample of the second group", "only active sample of a ray",
                   "ray without an active sample", "consecutive rays with 0, 1, 2, 3 active spans",
                   "transparent ray first in a walk", "transparent ray last in a walk", "two transparent rays in a row"}
    assert sum(int(fc.get_color_case(N, T).probe.sum()) >= 200 for N, T in DENSE) >= 5
    for N, T in fc.COLOR_WAVE_SHAPES:
        assert N > fc.RESIDENT_WAVES


def test_ragged_problem():
    c = fc.get_ragged_case()
    fc.check_discrimination(c)
    rays, M = c.rays, c.rows
    assert sorted(rays[:, 0]) == list(range(c.N)) and set(fc.RAGGED_COUNTS) >= {0, 1, 31, 32, 33, 1024, 1025}
    assert rays[fc.RAGGED_DROPPED, 1] + rays[fc.RAGGED_DROPPED, 2] > M
    owned = np.zeros(M, bool)
    for e, (rid, off, cnt) in enumerate(rays):
        if e != fc.RAGGED_DROPPED:
            assert not owned[off:off + cnt].any()
            owned[off:off + cnt] = True
    assert np.array_equal(owned, ~np.isnan(c.x[:, 0])) and (~owned).sum() > 50
    assert np.array_equal(np.abs(c.expected()["g_h16"][c.xrow, 0]), 2.0 * np.abs(c.tq)) and c.scale == 2.0


def test_periodic_forward_problem():
    N, T = fc.COLOR_FWD_STRIDE
    assert N * T > 2048 * 256 and np.gcd(fc.STRIDE_RAYS * T, 2048 * 256) == 1
    p = fc.TiledForward(N, T)
    o = p.tile(p.p.o)
    assert o.shape == (N * T, 2) and np.array_equal(o[:fc.STRIDE_RAYS * T], p.p.o) and np.array_equal(o[-T:], p.p.o[(N - 1) % fc.STRIDE_RAYS * T:][:T])
    fc.check_discrimination(p.p)


@pytest.mark.parametrize("T", fc.COMPOSITE_T)
def test_composite_problems(T):
    c = fc.get_composite_case(T)
    assert np.all((c.w == 0) | (c.w >= 1e-3)) and c.on.any() and not c.on[min(1, c.N - 1)].any() or T == 1
    assert np.array_equal(np.take_along_axis(c.sigma_pt, c.c.perm, axis=1), c.sigma_m)
    assert np.all(np.diff(c.z, axis=1) > 0) or T == 1


def test_direction_term_problems():
    for N in sorted(set(fc.DIR_N + fc.DIRB_N)):
        for K in fc.DIR_K:
            for ldw in (K + 15, K + 22):
                d = fc.get_dir_case(N, K, ldw)
                assert np.array_equal(d.cdir, np.rint(d.cdir)) and np.isnan(d.w0[:, K:]).all()


def test_broken_problems_are_rejected():
    c = fc.ColorCase(3, 64, seed=3)
    fc.check_conditions(c)
    c.weights[c.pos[0]] = 1.5e-4
    with pytest.raises(AssertionError):
        fc.check_conditions(c)
    c = fc.ColorCase(3, 64, seed=3)
    m = np.flatnonzero(c.probe)[0]
    c.g_rgb[c.pos[m]] = c.t[m]  # an uncompensated gradient: t s (1 - s) is no integer
    with pytest.raises(AssertionError, match="compensated"):
        c.expected()
    c = fc.ColorCase(3, 64, seed=3)
    c.x[c.xrow[5], 3] = 300.0
    with pytest.raises(AssertionError, match="exactness"):
        fc.check_conditions(c)
    # probes at |o| <= 6 would not survive the perturbed sigmoid in fp16
    o = np.array([[6.0, 6.0]])
    s = fc.sigmoid(o)
    g = (4.0 / (s * (1 - s))).astype(np.float32).astype(np.float64)
    sp = s * (1 + fc.S_PERTURB)
    assert not np.array_equal(fc.round16(g * sp * (1 - sp), False), [[4.0, 4.0]])
