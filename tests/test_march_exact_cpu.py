"""The conditions behind tests/test_march_exact_gpu.py, asserted without a GPU (tests/march_exact_cases.py):

Margin, termination and the oracle comparison cover every input a GPU launch takes: the twelve cases, their noise-0 forms (alive rounds) and their 72
serial-template forms.

- every case ends in the model, in the wave emulator and in the C oracle, under iteration guards, with at most 4096 lattice
  points per ray, finite or NaN `far`, finite origins and directions;
- MARGIN: every float32 decision the kernel takes on a case (level from the position, level from dt, the three cell
  coordinates, the first lattice point behind an exit) keeps at least 8 times the worst error of its float32 expression
  from the alternative.  The smallest ratio of every case is printed (the least: 28.7, case levels3);
- COVERAGE: every item of march_exact_cases.PROMISED (an explicit list: an item nothing reaches stands at 0), from the
  model's bookkeeping of lattice index // 64 and % 64;
- TEETH: the emulator without a mistake equals the model on every case (training walk and alive rounds of every n_step); each
  named mistake changes an expected array of at least one case — printed as a table.  One mistake cannot (see
  march_exact_cases.OUTPUT_NEUTRAL): it is held to the number of chunks the emulator probes;
- BLINDNESS: in the profile of the older marcher tests (H = 128, max_steps = 1024, C <= 2) no empty cell holds 64 lattice
  points, so no chunk lies inside one and the whole-chunk mistakes change nothing there;
- ORACLE: c_oracle.march_rays_train (base and noise-0 forms) and c_oracle.march_rays equal the model on every case: counts and deltas bit for bit,
  dirs, and xyzs as correctly rounded clip(o + t d).
"""
import math

import numpy as np
import pytest

import march_exact_cases as mc
from oracle import c_oracle

F = np.float32
NAMES = mc.case_names()


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _variant(name, kind):
    """A case as it goes to the GPU: the base case, its noise-0 form (alive rounds), or one of the six serial-template forms."""
    if kind == "base":
        return mc.cases()[name]
    return mc.lidar_case(name) if kind == "noise0" else mc.serial_case(name, *kind)


VARIANTS = ["base", "noise0"] + list(mc.SERIAL_KINDS)


@pytest.mark.parametrize("kind", VARIANTS, ids=str)
@pytest.mark.parametrize("name", NAMES)
def test_margin_and_termination(name, kind):
    """Every launch of the GPU file — base, noise-0 and serial-template inputs alike — keeps the margin and ends."""
    c = _variant(name, kind)
    name = c.name
    o, d, near, far, noise = c.arrays()
    assert np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(near).all() and (d != 0).any(axis=1).all()
    assert (np.isfinite(far) | np.isnan(far)).all(), "far is finite or NaN, never +inf"
    assert c.N <= 600 and c.grid.H in (8, 16) and c.grid.C in (1, 2, 3) and c.grid.bound in (1.0, 1.5, 2.0, 4.0)
    walks = mc.march_model(c, margins=True)           # (raises Hang where a guard trips)
    assert all(w.ratio is not None for w in walks)
    assert max(mc.case_ray(c, n).n_valid for n in range(c.N)) <= mc.MAX_LATTICE
    worst = min(w.ratio for w in walks)
    print(f"[march exact] {name}: {c.N} rays, {sum(len(w.idx) for w in walks)} samples, smallest margin ratio {worst:.3g}")
    assert worst >= 8, [n for n, w in enumerate(walks) if w.ratio < 8]


def test_the_case_list_covers_what_it_promises():
    cov = mc.coverage()
    for k in sorted(cov):
        print(f"[march exact] coverage {cov[k]:5d}  {k}")
    assert set(mc.PROMISED) <= set(cov) and len(mc.PROMISED) == 57
    assert not [k for k in mc.PROMISED if cov[k] == 0]


@pytest.mark.parametrize("name", NAMES)
def test_the_wave_replay_without_a_mistake_is_the_model(name):
    c = mc.cases()[name]
    want = mc.model_as_replay(c)
    got = mc.wave_replay(c)
    for n in range(c.N):
        assert got[n] != "hang" and (got[n][0], got[n][1]) == want[n], (name, n)
    lc = mc.lidar_case(name)
    for n_step in mc.N_STEPS_LIDAR:
        assert mc.wave_replay(lc, None, n_step) == mc.model_as_replay(lc, n_step), (name, n_step)


def test_every_mistake_shows():
    """mistake -> the number of cases (and rays) with a changed expected array; a walk that no longer ends counts."""
    table = {}
    for m in mc.MISTAKES:
        cases_changed = rays_changed = more_chunks = 0
        for name in NAMES:
            if m in mc.LIDAR_MISTAKES:
                c = mc.lidar_case(name)
                n = sum(mc.wave_replay(c, m, k) != mc.wave_replay(c, None, k) for k in (7, 64))
                rays_changed += n
                cases_changed += n > 0
                continue
            c = mc.cases()[name]
            base, got = mc.wave_replay(c), mc.wave_replay(c, m)
            ch = sum(g == "hang" or g[:2] != b[:2] for g, b in zip(got, base))
            more_chunks += sum(g != "hang" and g[2] > b[2] for g, b in zip(got, base))
            rays_changed += ch
            cases_changed += ch > 0
        table[m] = (cases_changed, rays_changed, more_chunks)
        print(f"[march exact] teeth {m:24s} cases changed {cases_changed:2d}  rays (lidar: n_step runs) {rays_changed:4d}  rays with more chunks {more_chunks}")
    for m, (cc, rr, ch) in table.items():
        if m in mc.OUTPUT_NEUTRAL:
            assert cc == 0 and ch >= 1, m            # no output can change (proof in march_exact_cases); the work does
        else:
            assert cc >= 1, m


@pytest.mark.parametrize("cascade", [1, 2])
def test_the_old_profile_cannot_see_the_whole_chunk_mistakes(cascade):
    worst, bound = mc.old_profile_points_per_empty_cell(cascade=cascade)
    print(f"[march exact] old profile C = {cascade}: at most {worst} lattice points in an empty cell (2^l max_steps / H = {bound:.0f})")
    assert 0 < worst <= bound < 64


def _check_samples(c, n, idx, xyz, dirs, deltas, what):
    _, d, _, _, _ = c.arrays()
    np.testing.assert_array_equal(_u32(deltas), _u32(mc.expected_rows(c, n, idx)), err_msg=f"{what}: deltas")
    np.testing.assert_array_equal(_u32(dirs), _u32(np.broadcast_to(d[n], (len(idx), 3))), err_msg=f"{what}: dirs")
    assert mc.xyz_is_correctly_rounded(c, n, idx, xyz), f"{what}: xyzs are not the correctly rounded clip(o + t d)"


@pytest.mark.parametrize("kind", ["base", "noise0"])
@pytest.mark.parametrize("name", NAMES)
def test_c_oracle_march_rays_train_equals_the_model(name, kind):
    c = _variant(name, kind)
    name = c.name
    walks = mc.march_model(c)
    o, d, near, far, noise = c.arrays()
    g = c.grid
    M = sum(len(w.idx) for w in walks) + 8
    xyzs, dirs, deltas, rays, counter = c_oracle.march_rays_train(o, d, g.bits, g.bound, c.dt_gamma, c.max_steps, g.C, g.H, M,
                                                                  near, far, noise)
    assert counter.tolist() == [M - 8, c.N]
    np.testing.assert_array_equal(rays[:, 0], np.arange(c.N))
    np.testing.assert_array_equal(rays[:, 2], [len(w.idx) for w in walks])
    for n, w in enumerate(walks):
        b, k = int(rays[n, 1]), int(rays[n, 2])
        _check_samples(c, n, w.idx, xyzs[b:b + k], dirs[b:b + k], deltas[b:b + k], f"{name} ray {n}")


@pytest.mark.parametrize("name", NAMES)
def test_c_oracle_march_rays_equals_the_model_from_a_chosen_start(name):
    for n_step, noise in mc.SERIAL_KINDS:
        c = mc.serial_case(name, n_step, noise)
        walks = mc.march_model(c)
        o, d, near, far, ns = c.arrays()
        g = c.grid
        xyzs, dirs, deltas = c_oracle.march_rays(c.N, n_step, np.arange(c.N), near, o, d, g.bound, c.dt_gamma, c.max_steps, g.C,
                                                 g.H, g.bits, near, far, ns)
        for n, w in enumerate(walks):
            k, b = len(w.idx), n * n_step
            assert k <= n_step and (deltas[b + k:b + n_step] == 0).all(), (name, n_step, n)
            _check_samples(c, n, w.idx, xyzs[b:b + k], dirs[b:b + k], deltas[b:b + k], f"{name} n_step {n_step} ray {n}")
