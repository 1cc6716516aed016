"""Exact known-answer tests of every instantiation of the fused MFMA MLP kernels (csrc/mlp.hip, mlp_bwd*.hip, mlp_wide.hip,
mlp_wgrad.hip and their bf16 builds) through the C ABI.

The problems are integer-valued (tests/mlp_exact_cases.py): every product is exact in fp16, bf16 and fp32 and every sum stays
below 2^24, so each tensor a kernel writes has ONE right value whatever the tiling, the k enumeration or the order of the
sums — results are compared with torch.equal (signed zeros are equal), never within a bound.  tests/test_mlp_exact_cpu.py
asserts, for every shape used here, the conditions that make such a comparison meaningful.

Every call:
  * writes into buffers pre-filled with a sentinel (-320: no expected value reaches it) that carry 64 guard words of the same
    sentinel behind them — an unwritten element and a write past the end both show;
  * reads inputs (x, gy, forward_buffer, the operands of lnh_mlp_wgrad) that carry 64 rows of NaN behind row B — a tail tile
    that lets rows >= B into a sum turns the sum into NaN;
  * adds weight gradients to a gradient pre-filled with 2.0 (the ABI says ADDED);
  * is made twice, and both results must be bit-identical.
"""
import numpy as np
import pytest
import torch

import mlp_exact_cases as cases
from exact_util import GUARD, POISON_ROWS, SENT, Out, _dev, _poisoned, _twice  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = {"": torch.float16, "_bf16": torch.bfloat16}
SFX = list(DTYPES)


class Problem:
    """A case of mlp_exact_cases on the device, in one element type: poisoned inputs and the expected outputs."""

    def __init__(self, c, sfx):
        self.c, self.sfx, self.dt = c, sfx, DTYPES[sfx]
        dt, B = self.dt, c.B
        idx = None if c.P == B else torch.from_numpy(c.idx).cuda()
        rows = lambda a: _dev(a, dt) if idx is None else _dev(a, dt)[idx]
        self.B, self.in_dim, self.H, self.nhm, self.act = B, c.in_dim, c.hidden, c.nhm, c.act
        self.x = _poisoned(rows(c.x), c.in_dim)
        self.gy = _poisoned(rows(c.gy), 16)
        self.w, self.wt = _dev(c.flat_weights(), dt), _dev(c.flat_weights_t(), dt)
        self.want_y, self.want_gx = rows(c.y), rows(c.gx)
        self._rows = rows
        self.want_dW = [_dev(d, torch.float32) + 2.0 for d in c.dW]

    def want_fb(self):
        return torch.stack([self._rows(v) for v in self.c.fb])

    def want_gb(self):
        return torch.stack([self._rows(v) for v in self.c.gb])

    def shape_args(self):
        return (self.B, self.in_dim, 16, self.H, self.nhm)


def _call(name, *args):
    from gpu_util import call
    call(name, *[a.buf if isinstance(a, Out) else a for a in args])


def _wgrad_ws():
    from gpu_util import wgrad
    return wgrad()


def _forward(p, with_fb, what):
    def run():
        y = Out((p.B, 16), p.dt)
        fb = Out((p.nhm + 1, p.B, p.H), p.dt) if with_fb else None
        _call("lnh_mlp_forward" + p.sfx, p.x, p.w, *p.shape_args(), p.act, cases.ACT_NONE, fb, y)
        return y, fb
    y, fb = _twice(run)
    y.check(p.want_y, f"{what} y (forward_buffer {'passed' if with_fb else 'NULL'})")
    if with_fb:
        fb.check(p.want_fb(), f"{what} forward_buffer")


def _backward_one_kernel(p, with_gx, what):
    def run():
        gx = Out((p.B, p.in_dim), p.dt) if with_gx else None
        dw = Out((p.w.numel(),), torch.float32, fill=2.0)
        _call("lnh_mlp_backward" + p.sfx, p.gy, p.x, p.w, *p.shape_args(), p.act, cases.ACT_NONE, gx, dw, *_wgrad_ws())
        return gx, dw
    gx, dw = _twice(run)
    tag = f"{what} (grad_inputs {'passed' if with_gx else 'NULL'})"
    if with_gx:
        gx.check(p.want_gx, f"{tag} gx")
    dw.check(torch.cat([d.reshape(-1) for d in p.want_dW]), f"{tag} dW")


def _what(c, sfx):
    return f"in {c.in_dim} hidden {c.hidden} nhm {c.nhm} B {c.B} act {c.act} {'bf16' if sfx else 'fp16'}:"


def _check_narrow(c, sfx, forward_buffer=True, backward=True):
    p, what = Problem(c, sfx), _what(c, sfx)
    _forward(p, False, what)
    if forward_buffer:
        _forward(p, True, what)
    if backward:
        _backward_one_kernel(p, True, what)
        _backward_one_kernel(p, False, what)


def _backward_data(p, with_gx, what):
    fb_in = _poisoned(p.want_fb(), p.H)

    def run():
        gb = Out((p.nhm + 1, p.B, p.H), p.dt)
        gx = Out((p.B, p.in_dim), p.dt) if with_gx else None
        _call("lnh_mlp_backward_data" + p.sfx, p.gy, fb_in, p.wt, *p.shape_args(), p.act, gb, gx)
        return gb, gx
    gb, gx = _twice(run)
    tag = f"{what} backward_data (grad_inputs {'passed' if with_gx else 'NULL'})"
    gb.check(p.want_gb(), f"{tag} backward_buffer")
    if with_gx:
        gx.check(p.want_gx, f"{tag} gx")


def _wgrad_per_matrix(p, what):
    """dW of every matrix from the two buffers, one lnh_mlp_wgrad launch each, as ffmlp.py::_backward_wide forms them."""
    c = p.c
    for l in range(p.nhm + 2):
        G, A = p._rows(c.g_of[l]), p._rows(c.a_of[l])
        M, N = G.shape[1], A.shape[1]
        Gp, Ap = _poisoned(G, M), _poisoned(A, N)

        def run():
            dw = Out((M, N), torch.float32, fill=2.0)
            _call("lnh_mlp_wgrad" + p.sfx, Gp, Ap, p.B, M, N, dw, *_wgrad_ws())
            return (dw,)
        _twice(run)[0].check(p.want_dW[l], f"{what} lnh_mlp_wgrad of matrix {l} ({M} x {N})")


def _check_wide(c, sfx, weight_gradients=True):
    p, what = Problem(c, sfx), _what(c, sfx)
    _forward(p, True, what)
    _forward(p, False, what)
    _backward_data(p, True, what)
    _backward_data(p, False, what)
    if weight_gradients:
        _wgrad_per_matrix(p, what)


# ------------------------------------------------------------------------------------ narrow kernels: every instantiation
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("hidden,nhm", cases.NARROW_NETS)
def test_narrow_instantiation_matrix(hidden, nhm, sfx):
    """k_mlp_forward<IN_KS 1..4, HT, NHM, FAST / runtime-switch> and the one-kernel backward of the same shapes (ReLU and the
    ACT = -1 instance with activation None), every input_dim including the odd multiples of 16 whose last k-step is half
    masked: y, forward_buffer (passed and NULL), gx, dW, and the same dW with grad_inputs == NULL."""
    for in_dim in cases.NARROW_IN_DIMS:
        for act in cases.ACTS:
            _check_narrow(cases.get_case(in_dim, hidden, nhm, cases.NARROW_B, act), sfx)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("in_dim,hidden,nhm", cases.EDGE_SHAPES)
def test_batch_edges(in_dim, hidden, nhm, sfx):
    """B = 1, below one 16-point tile, and one either side of the 16 / 64 / 128 / 256-point tiles of the launchers."""
    for B in cases.EDGE_BATCHES:
        for act in cases.ACTS:
            _check_narrow(cases.get_case(in_dim, hidden, nhm, B, act), sfx)


@pytest.mark.parametrize("sfx", SFX)
def test_empty_batch_touches_nothing(sfx):
    dt = DTYPES[sfx]
    c = cases.get_case(32, 64, 1, 1, cases.ACT_RELU)
    p = Problem(c, sfx)
    y, fb, gx, gb = Out((1, 16), dt), Out((2, 1, 64), dt), Out((1, 32), dt), Out((2, 1, 64), dt)
    dw = Out((p.w.numel(),), torch.float32, fill=2.0)
    _call("lnh_mlp_forward" + sfx, p.x, p.w, 0, 32, 16, 64, 1, 0, 6, fb, y)
    _call("lnh_mlp_backward" + sfx, p.gy, p.x, p.w, 0, 32, 16, 64, 1, 0, 6, gx, dw, *_wgrad_ws())
    _call("lnh_mlp_forward" + sfx, p.x, p.w, 0, 32, 16, 256, 1, 0, 6, fb, y)
    _call("lnh_mlp_backward_data" + sfx, p.gy, p.x, p.w, 0, 32, 16, 256, 1, 0, gb, gx)
    _call("lnh_mlp_wgrad" + sfx, p.gy, p.x, 0, 16, 32, dw, *_wgrad_ws())
    torch.cuda.synchronize()
    for o in (y, fb, gx, gb):
        assert bool((o.buf == SENT).all())
    assert bool((dw.data() == 2.0).all()) and bool((dw.buf[dw.n:] == SENT).all())


# ------------------------------------------------------------------------------------ second grid-stride iteration
def _stride_case(name):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    i, h, n, B = cases.stride_cases(cus)[name]
    return cases.get_case(i, h, n, B, cases.ACT_RELU)


@pytest.mark.parametrize("sfx", SFX)
def test_grid_stride_narrow_backward(sfx):
    """More than kWgradMaxBlocks (512) steps of PB = 128 points: workgroups walk a second step (periodic rows)."""
    c = _stride_case("narrow_backward")
    assert c.B > 512 * 128
    p, what = Problem(c, sfx), _what(c, sfx)
    _backward_one_kernel(p, True, what)
    _backward_one_kernel(p, False, what)


@pytest.mark.parametrize("sfx", SFX)
def test_grid_stride_narrow_forward(sfx):
    """More than 2048 workgroups x 256 points, input_dim 16, no forward buffer."""
    c = _stride_case("narrow_forward")
    assert c.B > 2048 * 256 and c.in_dim == 16
    _forward(Problem(c, sfx), False, _what(c, sfx))


@pytest.mark.parametrize("sfx", SFX)
def test_grid_stride_wide_lds_staged_forward(sfx):
    """Hidden 256 with a hidden matrix staged in LDS: one workgroup per CU x 256 points, and 300 more."""
    c = _stride_case("wide_lds_forward")
    assert c.B > 256 * torch.cuda.get_device_properties(0).multi_processor_count and c.hidden == 256 and c.nhm > 0
    p, what = Problem(c, sfx), _what(c, sfx)
    _forward(p, True, what)
    _forward(p, False, what)


@pytest.mark.parametrize("sfx", SFX)
def test_grid_stride_wide_forward_and_backward_data(sfx):
    """More than 4096 workgroups x 256 points through the wide forward and lnh_mlp_backward_data (hidden 32, 3 matrices)."""
    c = _stride_case("wide")
    assert c.B > 4096 * 256 and (c.hidden, c.nhm) == (32, 3)
    p, what = Problem(c, sfx), _what(c, sfx)
    _forward(p, True, what)
    _backward_data(p, True, what)


# ------------------------------------------------------------------------------------ wide kernels
@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("hidden,nhm", cases.WIDE_NETS)
def test_wide_kernels(hidden, nhm, sfx):
    """csrc/mlp_wide.hip: hidden 128 / 256 with 0 / 1 / 3 hidden matrices (256 with none takes the branch of launch_wide_fwd
    that does not stage in LDS), hidden 32 / 64 with 3 and 14, and (256, 14), the most check_wide accepts; ReLU and None;
    y, every forward_buffer layer, every backward_buffer layer, gx (passed and NULL), then dW per matrix by lnh_mlp_wgrad."""
    for in_dim in cases.WIDE_IN_DIMS:
        for B in cases.WIDE_BATCHES:
            for act in cases.ACTS:
                _check_wide(cases.get_case(in_dim, hidden, nhm, B, act), sfx)


# ------------------------------------------------------------------------------------ lnh_mlp_wgrad alone
def _check_wgrad(c, M, N, sfx, Gp, Ap, want_full):
    G, A = _poisoned(Gp[:, :M].contiguous(), M), _poisoned(Ap[:, :N].contiguous(), N)

    def run():
        dw = Out((M, N), torch.float32, fill=2.0)
        _call("lnh_mlp_wgrad" + sfx, G, A, c.B, M, N, dw, *_wgrad_ws())
        return (dw,)
    _twice(run)[0].check(want_full[:M, :N].contiguous(), f"lnh_mlp_wgrad{sfx} M {M} N {N} B {c.B}")


def _wgrad_operands(c, sfx):
    idx = torch.from_numpy(c.idx).cuda()
    return _dev(c.G, DTYPES[sfx])[idx], _dev(c.A, DTYPES[sfx])[idx], _dev(c.dW, torch.float32) + 2.0


@pytest.mark.parametrize("sfx", SFX)
def test_wgrad_every_tile_plan(sfx):
    """All 256 (M, N) of multiples of 16 up to 256: every (RM, RN) plan, the two-stage 512-thread and the 1024-thread kernel."""
    c = cases.get_wgrad_case(cases.WGRAD_B)
    Gp, Ap, want = _wgrad_operands(c, sfx)
    for M in cases.WGRAD_DIMS:
        for N in cases.WGRAD_DIMS:
            _check_wgrad(c, M, N, sfx, Gp, Ap, want)


@pytest.mark.parametrize("sfx", SFX)
@pytest.mark.parametrize("M,N", cases.WGRAD_EDGE_SHAPES)
def test_wgrad_batch_edges(M, N, sfx):
    """One either side of the 64-row stage and of four stages (one workgroup's share), a single row, several workgroups."""
    for B in cases.WGRAD_EDGE_BATCHES:
        c = cases.get_wgrad_case(B)
        _check_wgrad(c, M, N, sfx, *_wgrad_operands(c, sfx))


# ------------------------------------------------------------------------------------ module route
def _module_run(c, in_dim, out_dim, hidden, layers, dt, **kw):
    from lidarnerf.ffmlp import FFMLP
    m = FFMLP(in_dim, out_dim, hidden, layers, **kw).cuda()
    with torch.no_grad():
        m.weights.copy_(_dev(c.flat_weights(), torch.float32))
    x = _dev(c.x, torch.float32).requires_grad_(True)
    with torch.autocast("cuda", dtype=dt):
        y = m(x)
    assert y.dtype == dt and y.shape == (c.B, out_dim)
    y.backward(_dev(c.gy[:, :out_dim], dt))
    return y.detach(), x.grad, m.weights.grad


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("in_dim,out_dim,hidden,layers", cases.MODULE_SHAPES)
def test_module_route(in_dim, out_dim, hidden, layers, dt):
    """FFMLP with integer weights under fp16 / bf16 autocast: hidden 16 (zero-padded onto the hidden-32 kernels, 5 outputs),
    64 (one-kernel backward) and 256 (backward-data + lnh_mlp_wgrad): y, x.grad and weights.grad exactly, twice."""
    c = cases.get_case(in_dim, hidden, layers - 1, cases.NARROW_B, cases.ACT_RELU, out_dim)
    runs = [_module_run(c, in_dim, out_dim, hidden, layers, dt) for _ in range(2)]
    y, gx, gw = runs[0]
    assert torch.equal(y, _dev(c.y[:, :out_dim], dt))
    assert torch.equal(gx, _dev(c.gx, torch.float32))
    assert torch.equal(gw, _dev(c.flat_dW(), torch.float32))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_module_gemm_chain_equals_fused_kernels(dt):
    """FFMLP(..., gemm_chain=True) at a shape the fused kernels serve: the library-GEMM chain must run (no fused launch) and
    give the same y, x.grad and weights.grad.  The chain's autograd stores weight gradients in the 16-bit element type, so
    this problem keeps |dW| <= 256 (asserted in tests/test_mlp_exact_cpu.py), where that storage is exact too."""
    from lidarnerf import _hip
    in_dim, out_dim, hidden, layers, B = cases.MODULE_CHAIN
    c = cases.get_case(in_dim, hidden, layers - 1, B, cases.ACT_RELU, out_dim)
    fused = _module_run(c, in_dim, out_dim, hidden, layers, dt)
    names = [n + s for n in ("lnh_mlp_forward", "lnh_mlp_backward") for s in SFX]
    _hip.enable_timers(names)
    chain = _module_run(c, in_dim, out_dim, hidden, layers, dt, gemm_chain=True)
    launches = _hip.disable_timers()
    assert not any(launches.get(n) for n in names), f"gemm_chain=True ran fused kernels: {sorted(launches)}"
    assert torch.equal(fused[0], _dev(c.y[:, :out_dim], dt)) and torch.equal(fused[2], _dev(c.flat_dW(), torch.float32))
    for a, b in zip(fused, chain):
        assert torch.equal(a, b)
