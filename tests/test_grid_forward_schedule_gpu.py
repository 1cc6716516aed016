"""Forward schedule of the grid encoder (lnh_grid_forward_set_schedule): paired levels whose workgroups alternate in blocks
must write exactly what the level-major order writes — every (level, chunk) once, nothing else.  Both orders come from the
same library; the outputs are pre-filled with NaN and followed by guard words, and compared bit for bit.  The row map's
scalar / shift paths are also checked against the unmapped forward of the same rows."""
import numpy as np
import pytest
import torch

from oracle import grid_ref

pytestmark = pytest.mark.gpu

H, CH = 16, 2
PLS = grid_ref.per_level_scale(32768, H, 16)  # the benchmark's geometry: base 16, finest 32768, 2^19 rows
S = float(np.log2(PLS))
GUARD = 64
G = 32  # the interleave block the cases below are sized around
# (max_pairs, block) compared with level-major order (0 pairs); the last one is the library's default
ORDERS = [(8, 32), (8, 8), (3, 128), (0xFFFFFFFF, 0)]


def _points(B, seed):
    """Ray-ordered points (consecutive samples along rays), a few of them outside [0,1]."""
    r = np.random.default_rng(seed)
    n_rays = -(-B // 64)
    o = r.random((n_rays, 1, 3), dtype=np.float32) * 0.2 + 0.4
    d = r.standard_normal((n_rays, 1, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.linspace(0.002, 0.6, 64, dtype=np.float32)[None, :, None]
    x = (o + d * t).reshape(-1, 3)[:B].astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _offsets(D, L, log2_rows=19):
    return torch.from_numpy(grid_ref.make_offsets(D, L, PLS, H, log2_rows))


def _table(off, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(int(off[-1]), CH, device="cuda", generator=g) - 0.5).to(dtype)


def _forward(x, tab, off, L, want_dy_dx=False, map_=None, B_all=None):
    """One forward into NaN-filled, guarded buffers; returns the flat buffers (guards included)."""
    from lidarnerf import _hip
    dt = _hip.dtype_code(tab.dtype)
    if map_ is None:
        B = x.shape[0]
        flat, out = _guarded((L, B, CH), tab.dtype)
        dflat, dy = _guarded((B, L * 3 * CH), tab.dtype) if want_dy_dx else (None, None)
        _hip.call("lnh_grid_encode_forward", x.data_ptr(), tab.data_ptr(), off.data_ptr(), out.data_ptr(), B, 3, CH, L, S, H,
                  _hip.ptr(dy), 0, 0, 0, dt)
        return flat, dflat
    B, T_cur, T_tot, slot_off = map_
    flat, out = _guarded((L, B_all, CH), tab.dtype)
    _hip.call("lnh_grid_encode_forward_mapped_ex", x.data_ptr(), tab.data_ptr(), off.data_ptr(), out.data_ptr(), B, T_cur,
              T_tot, slot_off, B_all, CH, L, S, H, 0, dt)
    return flat, None


def _both_orders(run):
    """run() under level-major order and under every order of ORDERS; returns the level-major result."""
    from lidarnerf import _hip
    lib = _hip.lib()
    try:
        lib.lnh_grid_forward_set_schedule(0, 0)
        ref = run()
        torch.cuda.synchronize()
        for pairs, block in ORDERS:
            lib.lnh_grid_forward_set_schedule(pairs, block)
            got = run()
            torch.cuda.synchronize()
            for r, g in zip(ref, got):
                if r is not None:
                    assert torch.equal(_bits(r), _bits(g)), (pairs, block)
    finally:
        lib.lnh_grid_forward_set_schedule(0xFFFFFFFF, 0)
    return ref


def _check_written(flat, n):
    assert not torch.isnan(flat[:n]).any(), "an output element was never written"
    assert torch.isnan(flat[n:]).all(), "guard words behind the output were overwritten"


@pytest.mark.parametrize("B", [1, 255, 256, 257, 256 * G - 1, 256 * G + 1, 20011])
def test_paired_order_matches_level_major(B):
    L = 16
    off = _offsets(3, L)
    x, tab = _points(B, B), _table(off, torch.float16)
    flat, _ = _both_orders(lambda: _forward(x, tab, off, L))
    _check_written(flat, L * B * CH)


@pytest.mark.parametrize("L,log2_rows", [(1, 19), (5, 14), (4, 19)])
def test_degenerate_level_sets(L, log2_rows):
    """One level; an odd count (a level stays unpaired; 2^14 rows make levels 1 .. 4 hashed); no hashed level at all."""
    off = _offsets(3, L, log2_rows)
    hashed = [int(off[l + 1] - off[l]) == 1 << log2_rows for l in range(L)]
    assert any(hashed) == (L == 5)
    B = 256 * 8 + 3
    x, tab = _points(B, L), _table(off, torch.float16)
    flat, _ = _both_orders(lambda: _forward(x, tab, off, L))
    _check_written(flat, L * B * CH)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_dtypes_and_dy_dx(dtype):
    L, B = 16, 256 * 8 + 77
    off = _offsets(3, L)
    x, tab = _points(B, 5), _table(off, dtype)
    flat, dflat = _both_orders(lambda: _forward(x, tab, off, L, want_dy_dx=True))
    _check_written(flat, L * B * CH)
    _check_written(dflat, B * L * 3 * CH)


@pytest.mark.parametrize("T_cur,slot_off", [(768, 0), (64, 768), (100, 0)])
def test_row_map(T_cur, slot_off):
    """(768, 832, 0): a workgroup lies inside one ray, the quotient is taken on the scalar unit; (64, 832, 768): a shift;
    100: the general division.  Rows outside the map stay NaN; rows inside equal the unmapped forward of the same points."""
    L, rays, T_tot = 16, 3, 832
    B_all, B = rays * T_tot, rays * T_cur
    off = _offsets(3, L)
    x_all, tab = _points(B_all, 11), _table(off, torch.float16)
    flat, _ = _both_orders(lambda: _forward(x_all, tab, off, L, map_=(B, T_cur, T_tot, slot_off), B_all=B_all))
    assert torch.isnan(flat[L * B_all * CH:]).all()
    rows = (torch.arange(rays, device="cuda")[:, None] * T_tot + slot_off + torch.arange(T_cur, device="cuda")[None]).reshape(-1)
    out = flat[:L * B_all * CH].view(L, B_all, CH)
    from lidarnerf import _hip
    _hip.lib().lnh_grid_forward_set_schedule(0, 0)
    try:
        want, _ = _forward(x_all[rows].contiguous(), tab, off, L)
    finally:
        _hip.lib().lnh_grid_forward_set_schedule(0xFFFFFFFF, 0)
    assert torch.equal(_bits(out[:, rows]), _bits(want[:L * B * CH].view(L, B, CH)))
    other = torch.ones(B_all, dtype=torch.bool, device="cuda")
    other[rows] = False
    assert torch.isnan(out[:, other]).all(), "a row outside the map was written"
