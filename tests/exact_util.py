"""Device-side discipline shared by the exact known-answer GPU tests (tests/test_mlp_exact_gpu.py,
tests/test_field_exact_gpu.py, tests/test_render_exact_gpu.py, tests/test_loss_exact_gpu.py, tests/test_optim_exact_gpu.py,
tests/test_ragged_exact_gpu.py, tests/test_march_exact_gpu.py):
sentinel-filled outputs with guard words, NaN rows behind inputs, calls made twice."""
import numpy as np
import torch

GUARD = 64         # sentinel words behind every output
POISON_ROWS = 64   # NaN rows behind every input
SENT = -320.0      # a bf16 / fp16 / fp32 value that no expected 16-bit value reaches (|expected| <= 256)
_INT = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


def _dev(a, dt):
    """Small-integer float64 array -> device tensor of type dt (exact)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dt)


def _poisoned(t, row_len):
    """A copy of `t` with POISON_ROWS rows of NaN behind its last element."""
    flat = torch.full((t.numel() + POISON_ROWS * row_len,), float("nan"), dtype=t.dtype, device="cuda")
    flat[:t.numel()] = t.reshape(-1)
    return flat


class Out:
    """An output buffer: `shape` elements of the sentinel (or `fill`), then GUARD sentinel words."""

    def __init__(self, shape, dt, fill=SENT):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD,), SENT, dtype=dt, device="cuda")
        if fill != SENT:
            self.buf[:self.n] = fill

    def data(self):
        return self.buf[:self.n].view(self.shape)

    def check(self, want, what):
        assert bool((self.buf[self.n:] == SENT).all()), f"{what}: guard words behind the buffer were overwritten"
        got = self.data()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements differ, first at {bad[0].tolist()}: "
                                 f"got {got[tuple(bad[0])].item()}, want {want[tuple(bad[0])].item()}")


def _twice(fn):
    """Run a call twice on fresh buffers; every output of both runs must hold the same bits.  Returns the first run's."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        if u is not None:
            assert torch.equal(u.buf.view(_INT[u.buf.dtype]), v.buf.view(_INT[v.buf.dtype])), "two identical calls gave different bits"
    return a
