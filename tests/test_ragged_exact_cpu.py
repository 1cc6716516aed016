"""The problems of tests/test_ragged_exact_gpu.py, checked without a GPU: the conditions that make a bit-for-bit comparison of the
ragged compositing kernels meaningful (tests/ragged_exact_cases.py: opaque / transparent samples, dyadic lattices, 2^24 quanta,
-ffp-contract=off), the closed forms against the restated semantics and the structural model, coverage of every count, position
class, round length and table feature, the stop margin and the teeth of the tier-B bounds, agreement with the float64 oracle
under autograd, and the sensitivity of the references to each classic mistake."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import ragged_exact_cases as rc
from oracle import render_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OUT = ("weights_sum", "depth", "image", "grad_sigmas", "grad_feats")


def test_library_is_built_without_fp_contraction():
    """The closed forms count one rounding per operation; expf is then the only operation IEEE does not pin."""
    spec = importlib.util.spec_from_file_location("lnh_build", os.path.join(ROOT, "lidar-nerf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "-ffp-contract=off" in mod.FLAGS and not any("fast-math" in f for f in mod.FLAGS)


def test_shared_constants_are_imported_not_copied():
    import render_exact_cases as render
    assert rc.U is render.U and rc.gamma is render.gamma and rc.EXPF_ULPS is render.EXPF_ULPS and rc.TINY is render.TINY


# ------------------------------------------------------------------------------------------------ tier A: the training compositor
@pytest.mark.parametrize("K", rc.K_SET)
@pytest.mark.parametrize("tid", rc.table_ids())
def test_tier_a_problems(tid, K):
    """Conditions (asserted by get_case), and three statements of the answer that must be the same numbers: the closed forms,
    the serial restatement in float32 AND in float64 (equal only if no operation rounds), the structural model."""
    c = rc.get_case(tid, K)
    for thr in rc.THRESHOLDS:
        for finals in (c.finals(), None):
            r32, r64 = rc.lidar_reference(c, thr, F, finals), rc.lidar_reference(c, thr, np.float64, finals)
            m = rc.simulate(c, thr, finals=finals if finals is not None else (r32["weights_sum"], r32["depth"], r32["image"]))
            for k in OUT:
                assert np.array_equal(r32[k].astype(np.float64), r64[k], equal_nan=True), (thr, k)
                assert np.array_equal(m[k], r32[k], equal_nan=True), (thr, k)
        e = rc.lidar_closed_forms(c, thr)
        r = rc.lidar_reference(c, thr, F, c.finals())
        for k in OUT:
            assert np.array_equal(np.asarray(e[k], F).astype(np.float64), e[k], equal_nan=True), (thr, k)
            assert np.array_equal(np.asarray(e[k], F), r[k], equal_nan=True), (thr, k)
    # the forward answers, as the issue words them
    r, z = rc.lidar_reference(c, 1e-4, F), c.z()
    for j in range(c.N):
        i = c.index[j]
        if c.role[j] in ("kept", "last") and c.i0[j] is not None:
            assert r["weights_sum"][i] == 1 and r["depth"][i] == F(z[c.offset[j] + c.i0[j]])
            assert np.array_equal(r["image"][i], c.feats[c.offset[j] + c.i0[j]].astype(F))
        else:
            assert r["weights_sum"][i] == 0 and r["depth"][i] == 0 and not r["image"][i].any()


@pytest.mark.parametrize("tid", rc.table_ids())
def test_written_elements(tid):
    """Which gradient elements are written is part of the answer."""
    c = rc.get_case(tid, 2)
    written = {thr: ~np.isnan(rc.lidar_reference(c, thr, F, c.finals())["grad_sigmas"]) for thr in rc.THRESHOLDS}
    for thr in rc.THRESHOLDS:
        assert not written[thr][c.owner < 0].any(), "rows nobody owns, the rows of a dropped and of an empty ray"
        assert np.array_equal(written[thr], ~np.isnan(rc.lidar_reference(c, thr, F, c.finals())["grad_feats"]).any(1))
    for j in range(c.N):
        if c.role[j] not in ("kept", "last"):
            continue
        s = slice(c.offset[j], c.offset[j] + c.count[j])
        through = c.count[j] if c.i0[j] is None else c.i0[j] + 1
        assert written[1e-4][s].sum() == through and written[1e-4][s][:through].all()
        assert written[0.0][s].all(), "T_thresh = 0: nothing is < 0, the whole ray is written"
        assert written[1.0][s].sum() == through, "T_thresh = 1: T = 1 is not < 1, a transparent ray does not stop"


def test_every_class_is_met():
    met = rc.coverage()
    assert met["count"] == set(rc.COUNTS) and met["N"] == set(rc.N_SET)
    assert met["i0"] == set(rc.I0_SET) | {"none", "count-1"}
    assert met["pair"] >= set(rc.ray_specs()), "every count with every position of the first opaque sample, on a kept ray"
    roles = met["roles"]
    for tid, (N, _) in enumerate(rc.table_specs()):
        if N >= 3:
            assert {"last", "dropped", "empty"} <= roles[tid]
    singles = [roles[tid] for tid, (N, _) in enumerate(rc.table_specs()) if N == 1]
    assert {"last"} in singles and {"dropped"} in singles and {"empty"} in singles
    # partly filled workgroups of four waves; W of the alive compositor and the chunks a call takes
    assert {N % rc.WG_RAYS for N in rc.N_SET} == {0, 1, 3}
    assert {rc.width_of(n) for n in rc.N_STEPS} == {1, 2, 4, 8, 32, 64}
    assert {-(-n // rc.width_of(n)) for n in rc.N_STEPS} == {1, 2, 3}
    # a second opaque sample directly behind i0 = 63 and 127: the first lane of a round entered on the carry T = 0
    hit = set()
    for tid in rc.table_ids():
        c = rc.get_case(tid, 1)
        for j in range(c.N):
            if c.role[j] in ("kept", "last") and c.i0[j] in (63, 127) and c.i0[j] + 1 < c.count[j]:
                assert c.sigma[c.offset[j] + c.i0[j] + 1] == rc.OPAQUE
                hit.add(c.i0[j])
    assert hit == {63, 127}


def test_broken_problems_are_rejected():
    for breaker in ("sigma", "delta", "xyz", "columns"):
        N, rows = rc.table_specs()[0]
        c = rc.RaggedCase(rows, 2, seed=0)
        c.check_conditions()
        if breaker == "sigma":
            c.sigma[c.sigma > 0] = 2.0 ** 12                     # expf(-4) is not the same on every implementation
        elif breaker == "delta":
            c.deltas[3, 0] = 2.0 ** -11
        elif breaker == "xyz":
            c.xyz[5, 1] += 2.0 ** -9
        else:
            c.deltas[7, 1] = c.deltas[7, 0]
        with pytest.raises(AssertionError):
            c.check_conditions()


# ------------------------------------------------------------------------------------------------ tier A: the alive-ray evaluation
@pytest.mark.parametrize("tid", rc.table_ids())
def test_alive_rounds_end_on_the_training_forward(tid):
    """DESIGN 3.2, exactly: cut into rounds of any n_step, the alive compositor ends on the bits of the training forward."""
    c = rc.get_case(tid, 1 + tid % 3)
    want = rc.lidar_reference(c, 1e-4, F)
    for n_step in rc.N_STEPS:
        e, calls = rc.alive_final(c, n_step)
        if e is None:
            assert not any(r in ("kept", "last", "empty") for r in c.role)
            continue
        for k in ("weights_sum", "depth", "image"):
            assert np.array_equal(e[k], want[k]), (n_step, k)
        assert calls >= 1 and not (e["rays_alive"] >= 0).any() or set(e["rays_alive"][e["rays_alive"] >= 0]) == {7}


def test_alive_rounds_meet_every_liveness_rule():
    met = set()
    for tid in rc.table_ids():
        c = rc.get_case(tid, 1 + tid % 3)
        for n_step in rc.N_STEPS:
            for p, e in rc.alive_rounds(c, n_step):
                n_alive = p["alive_count"]
                assert 0 < n_alive <= p["n_alive_max"]
                if n_alive < p["n_alive_max"]:
                    met.add("slots beyond the alive count")
                    assert np.array_equal(e["rays_alive"][n_alive:], p["rays_alive"][n_alive:])
                for n in range(n_alive):
                    i, _, cnt = (int(v) for v in p["rays"][n])
                    dead = e["rays_alive"][n] == -1
                    same = all(np.array_equal(e[k][i], p[k][i]) for k in ("weights_sum", "depth", "image", "trans"))
                    if cnt == 0:
                        met.add("count 0: dead, state untouched")
                        assert dead and same
                    elif cnt < n_step:
                        met.add("count < n_step: dead")
                        assert dead
                    elif not p["rays_t"][i] < rc.INF:
                        met.add("full round with the mark: dead")
                        assert dead
                    elif e["trans"][i] < F(1e-4):
                        met.add("stopped: dead")
                        assert dead
                    else:
                        met.add("full round: alive")
                        assert not dead and e["rays_alive"][n] == i
    assert met == {"slots beyond the alive count", "count 0: dead, state untouched", "count < n_step: dead",
                   "full round with the mark: dead", "stopped: dead", "full round: alive"}


@pytest.mark.parametrize("count_kind", rc.ALIVE_STATE_COUNTS)
@pytest.mark.parametrize("thr", rc.ALIVE_STATE_THRESHOLDS)
def test_alive_state_case(thr, count_kind):
    p, kinds = rc.alive_state_case(thr, count_kind)          # (asserts the exactness conditions)
    e32, e64 = rc.alive_model(p, F), rc.alive_model(p, np.float64)
    for k in ("weights_sum", "depth", "image", "trans"):
        assert np.array_equal(e32[k].astype(np.float64), e64[k]), k
    assert np.array_equal(e32["rays_alive"], e64["rays_alive"])
    n_alive = min(max(p["alive_count"], 0), p["n_alive_max"])
    assert n_alive == {"all": 25, "clipped": 25, "zero": 0, "negative": 0, "fewer": 21}[count_kind]
    assert np.array_equal(e32["rays_alive"][n_alive:], p["rays_alive"][n_alive:])
    touched = set()
    stops = []
    for n in range(n_alive):
        i, kind = int(p["rays"][n, 0]), kinds[n]
        dead = e32["rays_alive"][n] == -1
        same = all(np.array_equal(e32[k][i], np.asarray(p[k], F)[i]) for k in ("weights_sum", "depth", "image", "trans"))
        if kind == "stale":
            assert dead and int(p["rays_alive"][n]) != i
            continue
        touched.add(i)
        tr = F(p["trans"][i])
        if kind == "stop":
            stops.append(int(np.flatnonzero(p["sigmas"][n * 8:(n + 1) * 8])[0]))
            assert dead and e32["trans"][i] == 0 and e32["weights_sum"][i] == F(p["weights_sum"][i]) + 1
        elif kind == "tie_opaque" and thr == rc.TIE_ABOVE:       # stops on its first, transparent sample: trans stored, nothing added
            assert dead and e32["trans"][i] == F(rc.TIE) and same
        elif kind in ("half_opaque", "tie_opaque"):
            assert dead and e32["trans"][i] == 0 and e32["weights_sum"][i] == F(p["weights_sum"][i]) + tr
            assert e32["depth"][i] != F(p["depth"][i])
        elif kind == "tie_through":
            assert e32["trans"][i] == F(rc.TIE) and same
            assert dead == (thr == rc.TIE_ABOVE), "on the threshold a ray goes on; the float above stops it"
        elif kind in ("through", "half_through"):
            assert not dead and same
        elif kind in ("short", "marked", "empty"):
            assert dead and same
    if count_kind in ("all", "clipped"):
        assert sorted(stops) == list(range(8)), "eight groups that stop at lanes 0 .. 7 of their own group"
        assert len({n % 8 for n in range(16) if kinds[n] == "stop"}) >= 4, "at several places of a wave"
    for i in set(range(p["N"])) - touched:                   # rays no live slot names: untouched
        assert all(np.array_equal(e32[k][i], np.asarray(p[k], F)[i]) for k in ("weights_sum", "depth", "image", "trans"))


# ------------------------------------------------------------------------------------------------ tier A: compaction and RGB
def test_compaction_reference():
    assert set(rc.COMPACT_SIZES) == {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4096}
    for n in rc.COMPACT_SIZES:
        for pattern in rc.COMPACT_PATTERNS:
            lst = rc.compact_list(n, pattern)
            out, cnt = rc.compact_reference(lst, n, n)
            assert np.array_equal(out, lst[lst >= 0]) and cnt == int((lst >= 0).sum())
            if pattern.startswith("list") and n:
                assert cnt == 1 and out[0] == lst[0 if pattern == "list_first" else n - 1]
    lst = rc.compact_list(2049, "alternating")
    assert rc.compact_reference(lst, 5000, 1025)[1] == 513 and rc.compact_reference(lst, -4, 2049)[1] == 0


@pytest.mark.parametrize("N", rc.RGB_N)
def test_rgb_problems(N):
    c = rc.get_rgb_case(N)
    for thr in rc.THRESHOLDS:
        r32, r64 = rc.rgb_reference(c, thr, F, c.finals()), rc.rgb_reference(c, thr, np.float64, c.finals())
        for k in ("weights_sum", "depth", "image", "grad_sigmas", "grad_rgbs"):
            assert np.array_equal(r32[k].astype(np.float64), r64[k], equal_nan=True), (thr, k)
    r = rc.rgb_reference(c, 1e-4, F, c.finals())
    lidar = rc.lidar_reference(c, 1e-4, F, c.finals())
    assert np.array_equal(r["weights_sum"], lidar["weights_sum"]) and np.array_equal(r["image"], lidar["image"])
    assert np.array_equal(np.isnan(r["grad_sigmas"]), np.isnan(lidar["grad_sigmas"])), "written through the stop sample"
    for j in range(c.N):
        i = c.index[j]
        if c.role[j] in ("kept", "last") and c.i0[j] is not None:
            s = slice(c.offset[j], c.offset[j] + c.i0[j] + 1)
            assert r["depth"][i] == F(c.deltas[s, 1].sum()), "depth: the running sum of deltas[:, 1] up to i0"
        else:
            assert r["depth"][i] == 0


@pytest.mark.parametrize("n_alive", rc.RGB_N)
def test_rgb_alive_quirks(n_alive):
    """lnh_composite_rays as the reference has it: T = 1 - weights_sum BEFORE the sample."""
    a = rc.rgb_alive_case(n_alive)
    alive, state = [int(i) for i in a["ids"]], a["state"]
    seen = set()
    for call in a["calls"]:
        e32, out = rc.rgb_alive_model(a["n_step"], 1e-4, alive, call["sigmas"], call["rgbs"], call["deltas"], state, F)
        e64, out64 = rc.rgb_alive_model(a["n_step"], 1e-4, alive, call["sigmas"], call["rgbs"], call["deltas"], state, np.float64)
        assert np.array_equal(out, out64)
        for k in e32:
            assert np.array_equal(e32[k].astype(np.float64), e64[k]), k
        for n, i in enumerate(alive):
            kind, saturated = call["kind"][n], F(state["weights_sum"][i]) == 1
            moved = e32["rays_t"][i] != F(state["rays_t"][i])
            if saturated:                                        # T = 0 before its first sample: weight 0, dead, t not saved
                assert out[n] == -1 and not moved and e32["weights_sum"][i] == 1
                assert np.array_equal(e32["image"][i], np.asarray(state["image"], F)[i])
                seen.add("dies on the first sample of the next call")
            elif kind == "opaque_last":
                assert out[n] == i and moved and e32["weights_sum"][i] == 1
                seen.add("opaque at the last sample: alive")
            elif kind == "opaque_early":
                assert out[n] == -1 and not moved and e32["weights_sum"][i] == 1
                seen.add("opaque earlier: dead")
            elif kind == "ends":
                assert out[n] == -1 and not moved
                seen.add("delta 0: dead")
            else:
                assert out[n] == i and moved
                seen.add("transparent: alive")
        state = e32
        alive = [int(v) for v in out if v >= 0]
    want = {"opaque at the last sample: alive", "opaque earlier: dead", "delta 0: dead", "transparent: alive",
            "dies on the first sample of the next call"}
    assert seen == want if n_alive >= 4 else seen <= want


# ------------------------------------------------------------------------------------------------ tier B
def _autograd(c, T_thresh):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    sg, ft = t(c.sigma).requires_grad_(True), t(c.feats).requires_grad_(True)
    ws, dep, img = render_ref.composite_ragged(sg[:c.M], ft[:c.M], t(c.deltas)[:c.M], t(c.xyz)[:c.M], t(c.o), t(c.d),
                                               torch.from_numpy(c.rays), float(F(T_thresh)))
    ((ws * t(c.g_ws)).sum() + (dep * t(c.g_depth)).sum() + (img * t(c.g_image)).sum()).backward()
    return ws.detach().numpy(), dep.detach().numpy(), img.detach().numpy(), sg.grad.numpy(), ft.grad.numpy()


@pytest.mark.parametrize("K,seed", rc.TIER_B_SEEDS)
def test_tier_b_reference_margin_and_oracle(K, seed):
    """No T_{i+1} of any ray within 8 bounds of the threshold (so float32 takes the same stop decisions); the new float64
    reference agrees with oracle/render_ref.composite_ragged under autograd within 1e-12 sum |addends|; every bound is finite."""
    c = rc.get_tier_b(K, seed)
    b = rc.lidar_bounds(c, 1e-4)
    assert b["margin"] > 8, b["margin"]
    assert rc.rgb_bounds(rc.get_tier_b(3, 13), 1e-4)["margin"] > 8
    assert len(b["walks"]) == sum(r in ("kept", "last") and n > 0 for r, n in zip(c.role, c.count)), "no ray is left out"
    assert c.count.max() == 200 and len(c.first_surface) == 10
    rounds = set()
    for j, s1 in c.first_surface.items():                        # the second surface: the next round or the round after
        w = b["walks"][c.index[j]]
        assert 0.25 < w["Tn"][s1] < 0.35 and w["last"] == s1 + 100
        rounds.add((s1 + 100) // rc.ROUND - s1 // rc.ROUND)
    assert rounds == {1, 2}
    ws, dep, img, gs, gf = _autograd(c, 1e-4)
    written = ~np.isnan(b["grad_sigmas"])
    for index, w in b["walks"].items():
        A = np.abs(w["w"] * w["z"]).sum()
        assert abs(ws[index] - b["weights_sum"][index]) <= 1e-12 and abs(dep[index] - b["depth"][index]) <= 1e-12 * max(A, 1e-300)
        assert np.all(np.abs(img[index] - b["image"][index]) <= 1e-12)
    assert np.all(np.abs(gs[:c.M][written[:c.M]] - b["grad_sigmas"][:c.M][written[:c.M]]) <= 1e-12 * b["A_grad_sigmas"][:c.M][written[:c.M]])
    assert not gs[:c.M][~written[:c.M]].any(), "autograd gives no gradient where the kernel writes none"
    np.testing.assert_allclose(gf[:c.M][written[:c.M]], b["grad_feats"][:c.M][written[:c.M]], rtol=1e-12, atol=0)
    for k in ("d_weights_sum", "d_depth", "d_image"):
        assert np.isfinite(b[k]).all()
    assert np.isfinite(b["d_grad_sigmas"][written]).all() and np.isfinite(b["d_grad_feats"][written]).all()
    # the closed-form tier-A tables through the same bound code: an exact answer has a bound near zero
    a = rc.lidar_bounds(rc.get_case(0, 2), 1e-4, rc.get_case(0, 2).finals())
    assert np.nanmax(a["d_weights_sum"]) < 1e-6


def test_rgb_alive_tier_b_margin_and_float32_restatement():
    """lnh_composite_rays on general alpha, three calls: no T = 1 - weights_sum that the stop test looks at lies within 8 bounds
    of the threshold, rays of every fate occur, every bound is finite, and the float32 restatement of the loop takes the same
    decisions as the float64 one and stays inside the bounds (they are no vacuous numbers)."""
    a = rc.rgb_alive_tier_b(**rc.RGB_ALIVE_B)
    rounds, margin = rc.rgb_alive_bounds(a, 1e-4)
    assert margin > 8, margin
    assert len(rounds) == 3 and [len(r[0]) for r in rounds] == [40, 21, 9], "rays die in every call and some live through all"
    assert any((c["deltas"][:, 0] == 0).any() for c in a["calls"])
    state = {k: np.asarray(v, F) for k, v in a["state"].items()}
    for call, (alive, e, err, after) in zip(a["calls"], rounds):
        e32, out32 = rc.rgb_alive_model(a["n_step"], 1e-4, alive, call["sigmas"], call["rgbs"], call["deltas"], state, F)
        assert np.array_equal(out32, after) and (after >= 0).any() and (after < 0).any()
        for k in e:
            assert np.isfinite(err[k]).all()
            assert np.all(np.abs(e32[k] - e[k]) <= err[k]), k
            listed = np.zeros(a["N"], bool)
            listed[a["ids"]] = True
            assert not err[k][~listed].any(), "a ray no call names keeps its state: bound 0"
        state = e32
    assert err["weights_sum"].max() < 1e-5 and err["depth"].max() < 1e-5


def test_the_bounds_have_teeth_and_the_old_profile_is_blind():
    """Dropping ONE round's carry of Tc, dc or accc in front of the second surface moves the float64 answer of that ray by more
    than ten bounds — surfaces in the same round, in neighbouring rounds, two rounds apart —, while the profile the earlier
    tests draw (counts < 40) cannot see any of the three."""
    c = rc.teeth_table()
    b = rc.lidar_bounds(c, 1e-4)
    assert b["margin"] > 8
    finals = (b["weights_sum"], b["depth"], b["image"])
    base = rc.simulate(c, 1e-4, dtype=np.float64, finals=finals)
    for k in OUT:
        np.testing.assert_allclose(base[k], b[k], rtol=1e-11, atol=1e-13, equal_nan=True)
    gaps = set()
    for n, (s1, s2) in enumerate(rc.TEETH_PAIRS):
        j = 2 + n
        index, s = c.index[j], slice(c.offset[j], c.offset[j] + c.count[j])
        gaps.add(s2 // rc.ROUND - s1 // rc.ROUND)
        for carry in ("Tc", "dc", "accc"):
            m = rc.simulate(c, 1e-4, dtype=np.float64, finals=finals, drop=(carry, s2 // rc.ROUND))
            ratios = [np.nanmax(np.abs(m["grad_sigmas"][s] - base["grad_sigmas"][s]) / b["d_grad_sigmas"][s])]
            if carry == "Tc":
                ratios += [abs(m[k][index] - base[k][index]) / b["d_" + k][index] for k in ("weights_sum", "depth")]
            assert min(ratios) > 10, (s1, s2, carry, ratios)
    assert gaps == {0, 1, 2}
    old = rc.old_profile_table()
    assert old.count.max() < 40
    want = rc.simulate(old, 1e-4)
    for mistake in ("Tc_dropped", "dc_dropped", "accc_dropped"):
        m = rc.simulate(old, 1e-4, mistake)
        assert all(np.array_equal(m[k], want[k], equal_nan=True) for k in OUT), mistake
        new = rc.get_tier_b(2, 12)
        m, w = rc.simulate(new, 1e-4, mistake), rc.simulate(new, 1e-4)
        assert not all(np.array_equal(m[k], w[k], equal_nan=True) for k in OUT), mistake


@pytest.mark.parametrize("K,seed", rc.TIER_B_SEEDS)
def test_alive_reference_in_float64_is_the_training_reference(K, seed):
    """Cut into rounds, the float64 alive model ends on the float64 training forward (to float64 rounding): the GPU file holds
    both kernels to the same reference."""
    c = rc.get_tier_b(K, seed)
    want = rc.lidar_reference(c, 1e-4, np.float64)
    for n_step in (3, 24, 130):
        e, _ = rc.alive_final(c, n_step, dtype=np.float64)
        for k in ("weights_sum", "depth", "image"):
            np.testing.assert_allclose(e[k], want[k], rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------------ sensitivity
def _train_changes(mistake):
    n = 0
    for tid in rc.table_ids():
        c = rc.get_case(tid, 2)
        for thr in rc.THRESHOLDS:
            r, m = rc.lidar_reference(c, thr, F, c.finals()), rc.simulate(c, thr, mistake, finals=c.finals())
            n += sum(not np.array_equal(m[k], r[k], equal_nan=True) for k in OUT)
    return n


@pytest.mark.parametrize("mistake", rc.MISTAKES)
def test_the_reference_tells_each_classic_mistake_apart(mistake):
    if mistake == "rgb_depth_col0":
        c = rc.get_rgb_case(65)
        assert not np.array_equal(rc.rgb_reference(c, 1e-4, F)["depth"], rc.rgb_reference(c, 1e-4, F, mistake=mistake)["depth"])
    elif mistake == "compact_wave_order":
        lst = rc.compact_list(1025, "alternating")
        assert not np.array_equal(rc.compact_reference(lst, 1025, 1025)[0], rc.compact_reference(lst, 1025, 1025, mistake)[0])
        assert np.array_equal(rc.compact_reference(lst[:64], 64, 64)[0], rc.compact_reference(lst[:64], 64, 64, mistake)[0])
    elif mistake.startswith("alive_"):
        n = 0
        for thr in rc.ALIVE_STATE_THRESHOLDS:
            p, _ = rc.alive_state_case(thr, "all")
            a, b = rc.alive_model(p), rc.alive_model(p, mistake=mistake)
            n += sum(not np.array_equal(a[k], b[k]) for k in a)
        for tid in rc.table_ids():
            c = rc.get_case(tid, 1 + tid % 3)
            for n_step in (8, 64):
                for (p, a), (_, b) in zip(rc.alive_rounds(c, n_step), rc.alive_rounds(c, n_step, mistake=mistake)):
                    n += sum(not np.array_equal(a[k], b[k]) for k in a)
                    break                                        # (the first round: later ones follow another list)
        assert n > 0
    else:
        assert _train_changes(mistake) > 0


def test_the_model_without_a_mistake_is_the_reference():
    assert _train_changes(None) == 0
