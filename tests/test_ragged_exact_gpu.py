"""Known-answer tests of the compositing kernels of the occupancy-grid path, through the C ABI:
lnh_lidar_composite_rays_train_forward / _backward (one wave per ray; Tc, dc and accc carried between 64-sample rounds, a stop
ballot), lnh_lidar_composite_rays (the alive-ray evaluation: W = 1 .. 64 lanes per ray, transmittance carried from call to
call), lnh_alive_compact, and the reference-shaped lnh_composite_rays_train_forward / _backward and lnh_composite_rays.

TIER A (tests/ragged_exact_cases.py; conditions asserted on the CPU by tests/test_ragged_exact_cpu.py): every sample is
transparent (sigma = 0) or opaque (expf argument <= -1024: alpha = 1, T = 0 exactly), everything else lies on dyadic lattices, and
the backward is handed finals that are not the forward's.  Every output has ONE float32 value in any scan order and is compared
with torch.equal — and so is the SET of gradient elements a kernel writes (the buffers start as a sentinel).  The alive-ray
compositor, fed the same rays in rounds of n_step = 1 .. 130, must end on the bits of the training forward.
Discipline of tests/exact_util.py: sentinel-filled outputs with guard words, NaN rows behind every input, every call twice.

TIER B: the random profile of tests/test_occupancy_gpu.py with counts up to 200 and two-surface rays, against float64 within a
bound PER ELEMENT derived from the rounding model (ragged_exact_cases lidar_bounds / rgb_bounds / rgb_alive_bounds).  Each
test prints the largest error / bound it sees; it must not exceed 1.
MEASURED on an MI355X (E = 1.68), largest error / bound: training forward 0.305, grad_sigmas 0.350, grad_feats 0.422; alive
compositor 0.302; RGB training forward 0.262, grad_sigmas 0.151, grad_rgbs 0.422; lnh_composite_rays weights_sum 0.365, rays_t 0.277.
"""

import numpy as np
import pytest
import torch

import ragged_exact_cases as rc
from exact_util import SENT, Out, _poisoned, _twice

pytestmark = pytest.mark.gpu
F = np.float32
STATE = ("weights_sum", "depth", "image", "trans")


def _call(name, *args):
    from gpu_util import call
    call(name, *[a.buf if isinstance(a, Out) else a for a in args])


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _in(a, row_len):
    """A float32 input with NaN rows behind it."""
    return _poisoned(_f32(a), row_len)


def _i32(a, pad=64):
    a = np.asarray(a)
    t = torch.zeros(a.size + pad, dtype=torch.int32, device="cuda")
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a.reshape(-1), dtype=np.int32)).cuda()
    return t


def _filled(values, dt=torch.float32):
    """An in/out buffer: `values`, then guard words."""
    values = np.asarray(values)
    o = Out(values.shape, dt)
    o.data().copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32 if dt == torch.int32 else np.float32)).cuda())
    return o


def _twice_i(fn):
    """exact_util._twice for outputs that include an int32 buffer."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert torch.equal(u.buf.view(torch.int32), v.buf.view(torch.int32)), "two identical calls gave different bits"
    return a


def _want(a):
    """Expected float32 array; NaN = never written = still the sentinel."""
    return _f32(np.nan_to_num(np.asarray(a, np.float64), nan=SENT))


def _untouched(*outs):
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.buf == SENT).all()), "a refused or empty call wrote to an output"


# ================================================================================================ tier A: the training compositor
class Train:
    def __init__(self, c):
        self.c, K = c, c.K
        self.sigma, self.feats = _in(c.sigma, 1), _in(c.feats, K)
        self.deltas, self.xyz = _in(c.deltas, 2), _in(c.xyz, 3)
        self.o, self.d, self.rays = _in(c.o, 3), _in(c.d, 3), _i32(c.rays)
        self.g_ws, self.g_depth, self.g_image = _in(c.g_ws, 1), _in(c.g_depth, 1), _in(c.g_image, K)

    def forward_outs(self):
        c = self.c
        return Out((c.N,), torch.float32), Out((c.N,), torch.float32), Out((c.N, c.K), torch.float32)

    def backward_outs(self):
        c = self.c
        return Out((c.rows_total,), torch.float32), Out((c.rows_total, c.K), torch.float32)

    def forward(self, thr, N=None, K=None, null=None, outs=None):
        c = self.c
        N, K = c.N if N is None else N, c.K if K is None else K
        ws, dep, img = outs if outs is not None else self.forward_outs()
        a = [self.sigma, self.feats, self.deltas, self.xyz, self.o, self.d, self.rays, c.M, N, K, thr, ws, dep, img]
        if null is not None:
            a[null] = None
        _call("lnh_lidar_composite_rays_train_forward", *a)
        return ws, dep, img

    def backward(self, thr, finals, N=None, K=None, null=None, outs=None):
        c = self.c
        N, K = c.N if N is None else N, c.K if K is None else K
        gs, gf = outs if outs is not None else self.backward_outs()
        a = [self.g_ws, self.g_depth, self.g_image, self.sigma, self.feats, self.deltas, self.xyz, self.o, self.d, self.rays,
             finals[0], finals[1], finals[2], c.M, N, K, thr, gs, gf]
        if null is not None:
            a[null] = None
        _call("lnh_lidar_composite_rays_train_backward", *a)
        return gs, gf


def _finals(c, finals):
    return _in(finals[0], 1), _in(finals[1], 1), _in(finals[2], c.K)


@pytest.mark.parametrize("K", rc.K_SET)
@pytest.mark.parametrize("tid", rc.table_ids())
def test_train_forward_and_backward(tid, K):
    """Every table at T_thresh = 1e-4, 0 and 1: the three sums, every gradient element and the set of elements written."""
    c = rc.get_case(tid, K)
    p = Train(c)
    fin = _finals(c, c.finals())
    for thr in rc.THRESHOLDS:
        e = rc.lidar_reference(c, thr, F, c.finals())
        what = f"table {tid} (N = {c.N}, K = {K}), T_thresh = {thr}:"
        ws, dep, img = _twice(lambda: p.forward(thr))
        ws.check(_want(e["weights_sum"]), f"{what} weights_sum")
        dep.check(_want(e["depth"]), f"{what} depth")
        img.check(_want(e["image"]), f"{what} image")
        gs, gf = _twice(lambda: p.backward(thr, fin))
        gs.check(_want(e["grad_sigmas"]), f"{what} grad_sigmas")
        gf.check(_want(e["grad_feats"]), f"{what} grad_feats")


def test_train_refusals_and_no_rays():
    """K = 0, K = 4 and a null pointer raise and change no byte of the outputs the call was handed; N = 0 returns without
    touching them."""
    c = rc.get_case(0, 2)
    p = Train(c)
    fin = _finals(c, c.finals())
    fwd, bwd = p.forward_outs(), p.backward_outs()
    for K in (0, 4):
        with pytest.raises(RuntimeError, match="K must be"):
            p.forward(1e-4, K=K, outs=fwd)
        with pytest.raises(RuntimeError, match="K must be"):
            p.backward(1e-4, fin, K=K, outs=bwd)
        _untouched(*fwd, *bwd)
    for null in (0, 6, 12):                                      # sigmas, rays, depth (the other two outputs stay live)
        with pytest.raises(RuntimeError, match="null pointer"):
            p.forward(1e-4, null=null, outs=fwd)
        _untouched(*fwd)
    for null in (0, 9, 11, 17):                                  # grad_weights_sum, rays, depth, grad_sigmas
        with pytest.raises(RuntimeError, match="null pointer"):
            p.backward(1e-4, fin, null=null, outs=bwd)
        _untouched(*bwd)
    p.forward(1e-4, N=0, outs=fwd)
    p.backward(1e-4, fin, N=0, outs=bwd)
    _untouched(*fwd, *bwd)


# ================================================================================================ tier A: the alive-ray evaluation
def _alive_call(p, null=None, K=None, sink=None):
    """One lnh_lidar_composite_rays call on fresh copies of the state of `p`: (weights_sum, depth, image, trans, rays_alive).
    `sink` receives the buffers before the call is made (a refused call raises)."""
    K = p["K"] if K is None else K
    row = p["n_step"]
    ins = dict(count=_i32([p["alive_count"]]), rays_t=_in(p["rays_t"], 1), rays=_i32(p["rays"]),
               sigmas=_in(p["sigmas"], row), feats=_in(p["feats"], row * p["K"]), deltas=_in(p["deltas"], row * 2),
               xyzs=_f32(p["xyzs"]), o=_in(p["o"], 3), d=_in(p["d"], 3))

    def run():
        st = [_filled(np.asarray(p[k], F)) for k in STATE]
        alive = _filled(np.asarray(p["rays_alive"], np.int32), torch.int32)
        if sink is not None:
            sink[:] = st + [alive]
        a = [p["n_alive_max"], p["n_step"], p["N"], K, p["T_thresh"], ins["count"], alive, ins["rays_t"], ins["rays"],
             ins["sigmas"], ins["feats"], ins["deltas"], ins["xyzs"], ins["o"], ins["d"], st[0], st[1], st[2], st[3]]
        if null is not None:
            a[null] = None
        _call("lnh_lidar_composite_rays", *a)
        return st + [alive]
    return run


def _check_alive(outs, e, what):
    for o, k in zip(outs[:4], STATE):
        o.check(_f32(e[k]), f"{what} {k}")
    outs[4].check(torch.from_numpy(np.asarray(e["rays_alive"], np.int32)).cuda(), f"{what} rays_alive")


@pytest.mark.parametrize("n_step", rc.N_STEPS)
@pytest.mark.parametrize("tid", rc.table_ids())
def test_alive_rounds_end_on_the_bits_of_the_training_forward(tid, n_step):
    """The rays of a table in rounds of n_step (W = 1 .. 64, up to three chunks a call): state and alive list after EVERY call,
    and after the last one the same bits as lnh_lidar_composite_rays_train_forward on the whole rays."""
    c = rc.get_case(tid, 1 + tid % 3)
    outs = None
    for r, (p, e) in enumerate(rc.alive_rounds(c, n_step)):
        outs = _twice_i(_alive_call(p))
        _check_alive(outs, e, f"table {tid}, n_step {n_step}, call {r}:")
    if outs is None:
        return                                                   # (the table of one dropped ray: nothing is ever alive)
    ws, dep, img = Train(c).forward(1e-4)
    for o, t, k in zip(outs[:3], (ws, dep, img), STATE):
        assert torch.equal(o.data().view(torch.int32), t.data().view(torch.int32)), f"table {tid}, n_step {n_step}: {k} differs from the training forward"


@pytest.mark.parametrize("count_kind", rc.ALIVE_STATE_COUNTS)
@pytest.mark.parametrize("thr", rc.ALIVE_STATE_THRESHOLDS)
def test_alive_state_and_liveness(thr, count_kind):
    """Caller-made state: trans 1, 1/2, 2^-13 with running sums, the strict-< tie, eight groups of a wave that stop at lanes
    0 .. 7 next to groups that do not, a short, an empty, a marked and a stale slot; alive_count clipped, 0, negative, smaller."""
    p, _ = rc.alive_state_case(thr, count_kind)
    _check_alive(_twice_i(_alive_call(p)), rc.alive_model(p), f"state case {thr} / {count_kind}:")


def test_alive_refusals():
    """K = 0, K = 4 and null pointers raise; the state and the alive list the call was handed keep every byte."""
    p, _ = rc.alive_state_case(rc.TIE, "all")
    before = dict({k: np.asarray(p[k], F) for k in STATE}, rays_alive=p["rays_alive"])
    for K in (0, 4):
        sink = []
        with pytest.raises(RuntimeError, match="K must be"):
            _alive_call(p, K=K, sink=sink)()
        _check_alive(sink, before, f"refused K = {K}:")
    for null in (5, 6, 8, 9, 15, 18):                            # alive_count, rays_alive, rays, sigmas, weights_sum, trans
        sink = []
        with pytest.raises(RuntimeError, match="null"):
            _alive_call(p, null=null, sink=sink)()
        _check_alive(sink, before, f"refused null argument {null}:")


# ================================================================================================ tier A: compaction
def _compact(lst, count, n_max):
    lst_d, cnt_d = _i32(lst, pad=0) if len(lst) else _i32([-1], pad=0), _i32([count])

    def run():
        out, n = Out((max(n_max, 1),), torch.int32), Out((1,), torch.int32)
        _call("lnh_alive_compact", n_max, cnt_d, lst_d, out, n)
        return out, n
    return _twice_i(run)


@pytest.mark.parametrize("pattern", rc.COMPACT_PATTERNS)
@pytest.mark.parametrize("n", rc.COMPACT_SIZES)
def test_compact(n, pattern):
    lst = rc.compact_list(n, pattern)
    want, cnt = rc.compact_reference(lst, n, n)
    out, got = _compact(lst, n, n)
    full = np.full(max(n, 1), int(SENT), np.int32)
    full[:cnt] = want
    out.check(torch.from_numpy(full).cuda(), f"compact {n} {pattern}: list (slots behind the count stay)")
    got.check(torch.tensor([cnt], dtype=torch.int32, device="cuda"), f"compact {n} {pattern}: count")


@pytest.mark.parametrize("count,n_max", [(4096, 1025), (5000, 64), (2049, 1), (-1, 2049), (-(2 ** 31), 64), (0, 4096), (63, 4096)])
def test_compact_clips_the_count(count, n_max):
    lst = rc.compact_list(4096, "alternating")
    want, cnt = rc.compact_reference(lst, count, n_max)
    out, got = _compact(lst, count, n_max)
    full = np.full(n_max, int(SENT), np.int32)
    full[:cnt] = want
    out.check(torch.from_numpy(full).cuda(), f"compact count {count}, n_alive_max {n_max}: list")
    got.check(torch.tensor([cnt], dtype=torch.int32, device="cuda"), "count")


def test_compact_refusals():
    lst, cnt = _i32(rc.compact_list(64, "all")), _i32([64])
    out, n = Out((64,), torch.int32), Out((1,), torch.int32)
    with pytest.raises(RuntimeError, match="OTHER half"):
        _call("lnh_alive_compact", 64, cnt, lst, lst, n)
    with pytest.raises(RuntimeError, match="OTHER half"):
        _call("lnh_alive_compact", 64, cnt, lst, out, cnt)
    for null in range(1, 5):
        a = [64, cnt, lst, out, n]
        a[null] = None
        with pytest.raises(RuntimeError, match="null pointer"):
            _call("lnh_alive_compact", *a)
    _untouched(out, n)
    torch.cuda.synchronize()
    assert int(cnt[0]) == 64 and torch.equal(lst[:64].cpu(), torch.from_numpy(rc.compact_list(64, "all")))


# ================================================================================================ tier A: the RGB template
class Rgb:
    def __init__(self, c):
        self.c = c
        self.sigma, self.rgb, self.deltas, self.rays = _in(c.sigma, 1), _in(c.feats, 3), _in(c.deltas, 2), _i32(c.rays)
        self.g_ws, self.g_image = _in(c.g_ws, 1), _in(c.g_image, 3)

    def forward(self, thr, N=None):
        c = self.c
        ws, dep, img = Out((c.N,), torch.float32), Out((c.N,), torch.float32), Out((c.N, 3), torch.float32)
        _call("lnh_composite_rays_train_forward", self.sigma, self.rgb, self.deltas, self.rays, c.M, c.N if N is None else N, thr, ws, dep, img)
        return ws, dep, img

    def backward(self, thr, wsf, fin, N=None):
        c = self.c
        gs, gc = Out((c.rows_total,), torch.float32), Out((c.rows_total, 3), torch.float32)
        _call("lnh_composite_rays_train_backward", self.g_ws, self.g_image, self.sigma, self.rgb, self.deltas, self.rays, wsf, fin,
              c.M, c.N if N is None else N, thr, gs, gc)
        return gs, gc


@pytest.mark.parametrize("N", rc.RGB_N)
def test_rgb_train_forward_and_backward(N):
    """depth is the running sum of deltas[:, 1] up to i0; the backward writes through the stop sample and nothing behind it."""
    c = rc.get_rgb_case(N)
    p = Rgb(c)
    wsf, fin = _in(c.ws_final, 1), _in(c.fin, 3)
    for thr in rc.THRESHOLDS:
        e = rc.rgb_reference(c, thr, F, c.finals())
        what = f"rgb N = {N}, T_thresh = {thr}:"
        ws, dep, img = _twice(lambda: p.forward(thr))
        ws.check(_want(e["weights_sum"]), f"{what} weights_sum")
        dep.check(_want(e["depth"]), f"{what} depth")
        img.check(_want(e["image"]), f"{what} image")
        gs, gc = _twice(lambda: p.backward(thr, wsf, fin))
        gs.check(_want(e["grad_sigmas"]), f"{what} grad_sigmas")
        gc.check(_want(e["grad_rgbs"]), f"{what} grad_rgbs")
    _untouched(*p.forward(1e-4, N=0), *p.backward(1e-4, wsf, fin, N=0))
    with pytest.raises(RuntimeError, match="null pointer"):
        _call("lnh_composite_rays_train_forward", p.sigma, p.rgb, p.deltas, p.rays, c.M, c.N, 1e-4, None, None, None)


@pytest.mark.parametrize("n_alive", rc.RGB_N)
def test_rgb_alive_quirks(n_alive):
    """lnh_composite_rays, two calls: T = 1 - weights_sum taken BEFORE the sample, a ray opaque at the last sample of a round
    stays alive and saves rays_t, one opaque earlier or ended by deltas[:, 0] == 0 is marked dead and keeps its rays_t."""
    a = rc.rgb_alive_case(n_alive)
    n_step = a["n_step"]
    alive, state = [int(i) for i in a["ids"]], {k: np.asarray(v, F) for k, v in a["state"].items()}
    for r, call in enumerate(a["calls"]):
        e, out = rc.rgb_alive_model(n_step, 1e-4, alive, call["sigmas"], call["rgbs"], call["deltas"], state)
        sig, rgb, dl = _in(call["sigmas"], n_step), _in(call["rgbs"], n_step * 3), _in(call["deltas"], n_step * 2)
        lst = np.full(n_alive, 5, np.int32)
        lst[:len(alive)] = alive

        def run():
            st = {k: _filled(state[k]) for k in ("weights_sum", "depth", "image", "rays_t")}
            al = _filled(lst, torch.int32)
            _call("lnh_composite_rays", len(alive), n_step, 1e-4, al, st["rays_t"], sig, rgb, dl, st["weights_sum"], st["depth"], st["image"])
            return st["weights_sum"], st["depth"], st["image"], st["rays_t"], al
        outs = _twice_i(run)
        for o, k in zip(outs[:4], ("weights_sum", "depth", "image", "rays_t")):
            o.check(_f32(e[k]), f"rgb alive {n_alive}, call {r}: {k}")
        lst[:len(alive)] = out
        outs[4].check(torch.from_numpy(lst).cuda(), f"rgb alive {n_alive}, call {r}: rays_alive")
        state, alive = e, [int(v) for v in out if v >= 0]
        if not alive:
            break


# ================================================================================================ tier B
def _utilisation(got, want, bound, what):
    """Largest |got - want| / bound over the elements that are written (finite `want`); unwritten ones must hold the sentinel,
    a bound of 0 asks for the exact value."""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    written = ~np.isnan(want)
    assert np.all(got[~written] == SENT), f"{what}: an element nobody may write was written"
    assert np.isfinite(bound[written]).all() and np.isfinite(got[written]).all(), what
    err = np.abs(got - want)
    zero = written & (bound == 0)
    assert np.all(err[zero] == 0), f"{what}: {int((err[zero] != 0).sum())} elements with an exact answer are off"
    use = written & (bound > 0)
    if not use.any():
        return 0.0
    ratio = np.where(use, err / np.where(use, bound, 1.0), 0.0)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    share = float(ratio[at])
    print(f"[bound] {what}: max error / bound = {share:.3f} at {tuple(int(i) for i in at)} ({int(use.sum())} elements)")
    assert share <= 1.0, f"{what}: off by {share:.3f} times the derived bound at {at}: got {got[at]!r}, want {want[at]!r}"
    return share


def _np(o):
    return o.data().cpu().numpy()


def test_rgb_alive_within_the_derived_bounds():
    """lnh_composite_rays on the random profile, three calls on the state the kernel itself left (T = 1 - weights_sum is carried
    IN the state), the survivors compacted between the calls: rays_alive as integers after every call against the float64
    run of the loop (the stop margin is asserted on the CPU), every element of weights_sum, depth, image and rays_t under its
    own bound (ragged_exact_cases.rgb_alive_bounds) — 0 for a ray no call names."""
    a = rc.rgb_alive_tier_b(**rc.RGB_ALIVE_B)
    n_step = a["n_step"]
    rounds, _ = rc.rgb_alive_bounds(a, 1e-4)
    keys = ("weights_sum", "depth", "image", "rays_t")
    state = {k: np.asarray(a["state"][k], F) for k in keys}
    for r, (call, (alive, e, err, after)) in enumerate(zip(a["calls"], rounds)):
        sig, rgb, dl = _in(call["sigmas"], n_step), _in(call["rgbs"], n_step * 3), _in(call["deltas"], n_step * 2)
        lst = np.full(a["n_alive"], 5, np.int32)
        lst[:len(alive)] = alive

        def run():
            st = {k: _filled(state[k]) for k in keys}
            al = _filled(lst, torch.int32)
            _call("lnh_composite_rays", len(alive), n_step, 1e-4, al, st["rays_t"], sig, rgb, dl, st["weights_sum"], st["depth"], st["image"])
            return [st[k] for k in keys] + [al]
        outs = _twice_i(run)
        lst[:len(alive)] = after
        outs[4].check(torch.from_numpy(lst).cuda(), f"rgb alive tier B, call {r}: rays_alive")
        for o, k in zip(outs[:4], keys):
            assert bool((o.buf[o.n:] == SENT).all()), f"{k}: guard words overwritten"
            _utilisation(_np(o), e[k], err[k], f"rgb alive tier B, call {r}: {k}")
        state = {k: _np(o) for o, k in zip(outs[:4], keys)}


@pytest.mark.parametrize("K,seed", rc.TIER_B_SEEDS)
def test_train_within_the_derived_bounds(K, seed):
    """40 rays of up to 200 samples, ten of them with two surfaces 100 samples apart: forward against float64, then the backward
    handed the float32 sums of the reference, every written gradient element under its own bound."""
    c = rc.get_tier_b(K, seed)
    p = Train(c)
    fwd = rc.lidar_bounds(c, 1e-4)
    ws, dep, img = _twice(lambda: p.forward(1e-4))
    for o, k in zip((ws, dep, img), ("weights_sum", "depth", "image")):
        _utilisation(_np(o), fwd[k], fwd["d_" + k], f"train forward K = {K}: {k}")
    finals = tuple(fwd[k].astype(F) for k in ("weights_sum", "depth", "image"))
    b = rc.lidar_bounds(c, 1e-4, finals)
    gs, gf = _twice(lambda: p.backward(1e-4, _finals(c, finals)))
    _utilisation(_np(gs), b["grad_sigmas"], b["d_grad_sigmas"], f"train backward K = {K}: grad_sigmas")
    _utilisation(_np(gf), b["grad_feats"], b["d_grad_feats"], f"train backward K = {K}: grad_feats")


@pytest.mark.parametrize("n_step", [3, 24, 130])
@pytest.mark.parametrize("K,seed", rc.TIER_B_SEEDS)
def test_alive_within_the_derived_bounds(K, seed, n_step):
    """The alive-ray compositor on the same rays in rounds, held to the SAME float64 reference (not to the bits of the training
    forward: its per-round sums associate differently).  The host loop follows the float64 model's alive list; the stop
    margin (CPU file) makes the float32 decisions the same, which the alive list of every call confirms."""
    c = rc.get_tier_b(K, seed)
    state = None
    calls = 0
    for p, e in rc.alive_rounds(c, n_step, dtype=np.float64):
        if state is not None:
            p = dict(p, **state)
        outs = _alive_call(p)()
        outs[4].check(torch.from_numpy(np.asarray(e["rays_alive"], np.int32)).cuda(), f"alive K = {K}, n_step {n_step}, call {calls}: rays_alive")
        state = {k: _np(o) for o, k in zip(outs[:4], STATE)}
        calls += 1
    b = rc.lidar_bounds(c, 1e-4, extra_sum_roundings=calls)
    for k in ("weights_sum", "depth", "image", "trans"):         # trans: T behind the last sample that counts, 1 where none does
        _utilisation(state[k], b[k], b["d_" + k], f"alive K = {K}, n_step {n_step} ({calls} calls): {k}")
    # most rays end on a sample so dense that float32 has 1 - alpha = 0: trans is 0 there and the bound is the float64 value
    # itself (ratio 1.000).  The figure that says something comes from the rays that end on a representable 1 - alpha.
    rep = b["d_trans"] < 0.5 * b["trans"]
    assert rep.sum() >= 5
    _utilisation(state["trans"][rep], b["trans"][rep], b["d_trans"][rep], f"alive K = {K}, n_step {n_step}: trans where 1 - alpha is representable")


def test_rgb_within_the_derived_bounds():
    """The thread-per-ray training compositors on the random profile.  alpha is no output of these kernels, so expf cannot be separated
    from the rest of the chain and held exactly: the derived bound per element it is (ragged_exact_cases.rgb_bounds)."""
    c = rc.get_tier_b(3, 13)
    p = Rgb(c)
    fwd = rc.rgb_bounds(c, 1e-4)
    ws, dep, img = _twice(lambda: p.forward(1e-4))
    for o, k in zip((ws, dep, img), ("weights_sum", "depth", "image")):
        _utilisation(_np(o), fwd[k], fwd["d_" + k], f"rgb forward: {k}")
    finals = tuple(fwd[k].astype(F) for k in ("weights_sum", "depth", "image"))
    b = rc.rgb_bounds(c, 1e-4, finals)
    gs, gc = _twice(lambda: p.backward(1e-4, _in(finals[0], 1), _in(finals[2], 3)))
    _utilisation(_np(gs), b["grad_sigmas"], b["d_grad_sigmas"], "rgb backward: grad_sigmas")
    _utilisation(_np(gc), b["grad_rgbs"], b["d_grad_rgbs"], "rgb backward: grad_rgbs")
