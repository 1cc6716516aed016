"""Integer-valued known-answer problems for the fused MFMA MLP kernels (csrc/mlp*.hip), with their exact answers.

TEST INFRASTRUCTURE ONLY (no GPU).  Products of small integers are exact in fp16, bf16 and fp32, and integer sums below 2^24
are exact in fp32 in ANY order: an MLP whose inputs, weights, activations and gradients are all small integers has ONE right
answer for every tensor a kernel writes, whatever its tiling, k enumeration or summation tree.  The answers come from
oracle/mlp_ref.py in float64 with `half=False`.

A problem is a set of `P` distinct batch rows and an index vector: batch row b is period row `idx[b]` (`idx = arange(B)` for
the small batches, `arange(B) % 257` for the batches that reach a launcher's second grid-stride iteration: 257 is prime to
every tile size, the reference costs 257 rows, and the expected output is a tiling of them).

Recipe (`recipe="default"`): x and gy in {-1 .. 2}; W0 three +-1 per row; hidden matrices a permutation matrix plus one
extra +-1 per row for up to 4 hidden matrices, a plain permutation matrix for deeper nets; Wo max(6, hidden / 4) +-1 per row.
Rows that would make a condition fail (a dead ReLU row, a value past 256) are drawn again; `check_conditions` then ASSERTS
every condition on the reference alone, and `check_discrimination` asserts that the classic kernel mistakes (a dropped or
duplicated row, a dropped tile, a transposed matrix, swapped k or hidden indices, a lost weight tile) change an answer.
"""
import functools

import numpy as np

from oracle import mlp_ref

PERIOD = 257          # rows of a periodic batch
VALUE_LIMIT = 256.0   # integers up to 2^8 are bf16 values (8 significant bits), up to 2^11 fp16 values
SUM_LIMIT = 2.0 ** 24  # integer sums below it are exact in fp32 in any order
ACT_RELU, ACT_NONE = mlp_ref.ACT_RELU, mlp_ref.ACT_NONE

# ------------------------------------------------------------------------------------------------ the shapes of the GPU file
NARROW_IN_DIMS = (16, 32, 48, 64, 80, 96, 112, 128)
NARROW_NETS = [(h, n) for h in (32, 64) for n in (0, 1, 2)]          # (hidden, n_hidden_mats)
NARROW_B = 129
EDGE_SHAPES = [(32, 64, 1), (48, 32, 2)]                              # (input_dim, hidden, n_hidden_mats)
EDGE_BATCHES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ACTS = (ACT_RELU, ACT_NONE)
WIDE_NETS = [(h, n) for h in (128, 256) for n in (0, 1, 3)] + [(h, n) for h in (32, 64) for n in (3, 14)] + [(256, 14)]
WIDE_IN_DIMS = (16, 48, 128)
WIDE_BATCHES = (1, 65, 257)
WGRAD_DIMS = tuple(range(16, 257, 16))
WGRAD_B = 193
WGRAD_EDGE_SHAPES = [(64, 48), (256, 256), (16, 256)]
WGRAD_EDGE_BATCHES = (1, 63, 64, 65, 255, 256, 257, 1025)
MODULE_SHAPES = [(32, 5, 16, 2), (48, 16, 64, 3), (32, 3, 256, 2)]    # (input_dim, output_dim, hidden, num_layers)
MODULE_CHAIN = (48, 16, 64, 3, 17)                                    # (..., B): FFMLP(gemm_chain=True) against the fused kernels
MI355X_CUS = 256


def stride_cases(cus=MI355X_CUS):
    """name -> (input_dim, hidden, n_hidden_mats, B): one batch past the first grid-stride iteration of every launcher."""
    return {
        "narrow_backward": (32, 64, 1, 512 * 128 + 129),      # kWgradMaxBlocks workgroups x PB = 128 points
        "narrow_forward": (16, 64, 1, 2048 * 256 + 65),       # 2048 workgroups x 256 points
        "wide_lds_forward": (48, 256, 1, 256 * cus + 300),    # one 512-thread workgroup per CU x 256 points
        "wide": (16, 32, 3, 4096 * 256 + 65),                 # 4096 workgroups x 256 points (forward and backward-data)
    }


def all_mlp_cases(cus=MI355X_CUS):
    """Every (input_dim, hidden, n_hidden_mats, B, act, out_cols) the GPU file builds a problem for."""
    out = []
    for h, n in NARROW_NETS:
        for i in NARROW_IN_DIMS:
            out += [(i, h, n, NARROW_B, a, 16) for a in ACTS]
    for i, h, n in EDGE_SHAPES:
        out += [(i, h, n, B, a, 16) for B in EDGE_BATCHES for a in ACTS]
    for i, h, n, B in stride_cases(cus).values():
        out.append((i, h, n, B, ACT_RELU, 16))
    for h, n in WIDE_NETS:
        out += [(i, h, n, B, a, 16) for i in WIDE_IN_DIMS for B in WIDE_BATCHES for a in ACTS]
    for i, o, h, layers in MODULE_SHAPES:
        out.append((i, h, layers - 1, NARROW_B, ACT_RELU, o))
    i, o, h, layers, B = MODULE_CHAIN
    out.append((i, h, layers - 1, B, ACT_RELU, o))
    return out


# ------------------------------------------------------------------------------------------------ generator
def _distinct_rows(draw):
    """Two equal rows of a matrix are two equal hidden units: swapping them would change nothing.  Draw until none are."""
    while True:
        W = draw()
        if len(np.unique(W, axis=0)) == len(W):
            return W


def _sparse_rows(r, rows, cols, k):
    """k entries of +-1 in every row, all rows distinct (rows that repeat an earlier one are drawn again)."""
    k = min(k, cols)
    W = np.zeros((rows, cols))
    todo = np.arange(rows)
    while len(todo):
        j = np.argsort(r.random((len(todo), cols)), axis=1)[:, :k]
        W[todo] = 0.0
        W[todo[:, None], j] = r.choice([-1.0, 1.0], size=j.shape)
        _, first = np.unique(W, axis=0, return_index=True)
        todo = np.setdiff1d(np.arange(rows), first)
    return W


def _hidden_matrix(r, H, kind):
    if kind != "perm+1":  # (the rows of a permutation matrix are distinct as they are)
        return _hidden_matrix_once(r, H, kind)
    return _distinct_rows(lambda: _hidden_matrix_once(r, H, kind))


def _hidden_matrix_once(r, H, kind):
    W = np.zeros((H, H))
    perm = r.permutation(H)
    rows = np.arange(H)
    if kind == "signed":  # the BAD recipe: one +-1 per row — half of a ReLU layer's units die in every layer
        W[rows, perm] = r.choice([-1.0, 1.0], size=H)
        return W
    W[rows, perm] = 1.0
    if kind == "perm+1":
        W[rows, (perm + 1 + r.integers(0, H - 1, size=H)) % H] = r.choice([-1.0, 1.0], size=H)
    return W


def make_weights(r, in_dim, hidden, nhm, recipe="default"):
    kind = "signed" if recipe == "signed_sparse_hidden" else ("perm+1" if nhm <= 4 else "perm")
    mats = [_sparse_rows(r, hidden, in_dim, 3)]
    mats += [_hidden_matrix(r, hidden, kind) for _ in range(nhm)]
    mats.append(_sparse_rows(r, 16, hidden, max(6, hidden // 4)))
    return mats


class Case:
    """x [P, in], gy [P, 16], mats, idx [B] -> the exact y, fb[l], gb[l], gx (period rows) and dW[l] (whole batch)."""

    def __init__(self, x, gy, mats, idx, act, verify=True):
        self.x, self.gy, self.mats, self.idx, self.act = x, gy, mats, idx, act
        self.B, self.P = len(idx), len(x)
        self.in_dim, self.hidden, self.nhm = x.shape[1], mats[0].shape[0], len(mats) - 2
        self.cnt = np.bincount(idx, minlength=self.P).astype(np.float64)  # how often a period row occurs in the batch
        self.y, self.fb = mlp_ref.mlp_forward(x, mats, act=act, half=False)
        gx, dws = mlp_ref.mlp_backward(x, mats, gy, act=act, half=False) if verify else (None, None)
        # gradient w.r.t. the pre-activation of every hidden layer: what lnh_mlp_backward_data writes to backward_buffer[l]
        self.gb, g = [None] * (self.nhm + 1), gy
        for k in range(self.nhm + 1, 0, -1):
            g = mlp_ref.act_backward_from_post(act, g @ mats[k], self.fb[k - 1])
            self.gb[k - 1] = g
        self.gx = self.gb[0] @ mats[0]
        assert not verify or np.array_equal(self.gx, gx), "per-layer gradients disagree with mlp_ref.mlp_backward"
        self.g_of = self.gb + [gy]       # gradient at the output of matrix l
        self.a_of = [x] + self.fb        # input of matrix l
        self.dW = [(self.g_of[l] * self.cnt[:, None]).T @ self.a_of[l] for l in range(self.nhm + 2)]
        if verify and self.P == self.B and np.array_equal(idx, np.arange(self.B)):
            assert all(np.array_equal(a, b) for a, b in zip(self.dW, dws)), "weight gradients disagree with mlp_ref.mlp_backward"

    def compared(self):
        """name -> every tensor a GPU test compares (16-bit storage), period rows."""
        t = {"y": self.y, "gx": self.gx}
        t.update({f"fb{l}": v for l, v in enumerate(self.fb)})
        t.update({f"gb{l}": v for l, v in enumerate(self.gb)})
        return t

    def flat_weights(self):
        return np.concatenate([m.ravel() for m in self.mats])

    def flat_weights_t(self):
        return np.concatenate([np.ascontiguousarray(m.T).ravel() for m in self.mats])

    def flat_dW(self):
        return np.concatenate([d.ravel() for d in self.dW])


def _bad_rows(c):
    """Period rows that would fail a per-row condition."""
    bad = np.zeros(c.P, bool)
    for t in [c.x, c.gy] + list(c.compared().values()):
        bad |= ~np.any(t != 0, axis=1)
        bad |= np.any(np.abs(t) > VALUE_LIMIT, axis=1)
    return bad


def build_case(in_dim, hidden, nhm, B, act=ACT_RELU, out_cols=16, recipe="default", lo=-1, hi=2, seed=0):
    P = min(B, PERIOD)
    idx = np.arange(B) % P
    r = np.random.default_rng([in_dim, hidden, nhm, B, act, out_cols, seed])
    mats = make_weights(r, in_dim, hidden, nhm, recipe)
    mats[-1][out_cols:] = 0.0

    def draw(n):
        x = r.integers(lo, hi + 1, size=(n, in_dim)).astype(np.float64)
        gy = np.zeros((n, 16))
        gy[:, :out_cols] = r.integers(lo, hi + 1, size=(n, out_cols))
        return x, gy
    x, gy = draw(P)
    for _ in range(16):  # rows that break a condition are drawn again; what is left after that fails check_conditions
        c = Case(x, gy, mats, idx, act)
        bad = _bad_rows(c)
        if not bad.any():
            break
        x[bad], gy[bad] = draw(int(bad.sum()))
    c = Case(x, gy, mats, idx, act)
    c.out_cols = out_cols
    return c


def check_conditions(c):
    """The conditions of an exact test, asserted on the reference alone."""
    tensors = dict(c.compared(), x=c.x, gy=c.gy, **{f"W{l}": m for l, m in enumerate(c.mats)})
    for name, t in tensors.items():
        assert np.all(np.abs(t) <= VALUE_LIMIT), f"exactness: |{name}| reaches {np.abs(t).max()} > {VALUE_LIMIT}"
        assert np.array_equal(mlp_ref.round_bf16(t).astype(np.float64), t), f"exactness: {name} is not a bf16 tensor"
        assert np.array_equal(t.astype(np.float16).astype(np.float64), t), f"exactness: {name} is not an fp16 tensor"
    for l in range(c.nhm + 2):
        g, a = c.g_of[l], c.a_of[l]
        bound = (np.abs(g) * c.cnt[:, None]).T @ np.abs(a)
        assert bound.max() < SUM_LIMIT, f"dW sum bound: matrix {l} sums |terms| up to {bound.max()} >= 2^24"
        assert np.all(np.any(g != 0, axis=1)), f"every batch row counts: the gradient of matrix {l} has an all-zero row"
        assert np.all(np.any(a != 0, axis=1)), f"every batch row counts: the input of matrix {l} has an all-zero row"
        d = c.dW[l]
        tiles = np.abs(d).reshape(d.shape[0] // 16, 16, d.shape[1] // 16, 16).max(axis=(1, 3))
        assert np.all(tiles > 0), f"every tile counts: dW{l} has an all-zero 16x16 tile"
    assert np.all(np.any(c.y != 0, axis=1)) and np.all(np.any(c.gx != 0, axis=1)), "an output row of y or gx is all zero"


def _differs(c, m):
    """Does the mutated problem `m` (same batch size) change a compared tensor or a weight gradient?"""
    for k, v in c.compared().items():
        if not np.array_equal(v[c.idx], m.compared()[k][m.idx]):
            return True
    return any(not np.array_equal(a, b) for a, b in zip(c.dW, m.dW))


def check_discrimination(c, seed=0):
    """Each classic kernel mistake, applied to the reference, must change at least one compared tensor."""
    r = np.random.default_rng(seed)
    redo = lambda **kw: Case(kw.get("x", c.x), kw.get("gy", c.gy), kw.get("mats", c.mats), kw.get("idx", c.idx), c.act, verify=False)

    def dW_with(idx):
        cnt = np.bincount(idx, minlength=c.P).astype(np.float64)
        return [(c.g_of[l] * cnt[:, None]).T @ c.a_of[l] for l in range(c.nhm + 2)]
    # a dropped row / tile shows in EVERY weight gradient (its rows of y, gx stay unwritten: the sentinel shows those)
    for what, keep in (("last batch row", c.B - 1), ("last 16-row tile", (c.B - 1) // 16 * 16)):
        for l, (a, b) in enumerate(zip(c.dW, dW_with(c.idx[:keep]))):
            assert not np.array_equal(a, b), f"discrimination: dropping the {what} leaves dW{l} unchanged"
    if c.B > 1:
        idx = c.idx.copy()
        idx[-1] = idx[0]
        assert not np.array_equal(c.y[c.idx], c.y[idx]) and not np.array_equal(c.gx[c.idx], c.gx[idx]), \
            "discrimination: row 0 duplicated into the last row changes neither y nor gx"
        for l, (a, b) in enumerate(zip(c.dW, dW_with(idx))):
            assert not np.array_equal(a, b), f"discrimination: row 0 duplicated into the last row leaves dW{l} unchanged"
    for m in range(c.nhm if c.nhm <= 3 else 0, 0, -1):
        mats = list(c.mats)
        mats[m] = np.ascontiguousarray(mats[m].T)
        assert _differs(c, redo(mats=mats)), f"discrimination: hidden matrix {m} transposed changes nothing"
    if c.nhm > 3:  # (deep nets: one matrix from each end and the middle)
        for m in (1, c.nhm // 2, c.nhm):
            mats = list(c.mats)
            mats[m] = np.ascontiguousarray(mats[m].T)
            assert _differs(c, redo(mats=mats)), f"discrimination: hidden matrix {m} transposed changes nothing"
    # Index swaps.  From 16 batch rows on EVERY probed pair must show; a batch of fewer rows cannot tell all pairs apart (one
    # row of {-1 .. 2} has x[k] == x[k + 8] for a quarter of the k), so there at least one probed pair of each kind must: the
    # index paths themselves are the same at every batch size and are pinned by the larger batches of the same shape.
    need = all if c.B >= 16 else any

    def swapped_x(k, d):
        x = c.x.copy()
        x[:, [k, k + d]] = x[:, [k + d, k]]
        return _differs(c, redo(x=x))

    def swapped_units(l, h):
        mats = list(c.mats)
        mats[l] = mats[l].copy()
        mats[l][[h, h + 16]] = mats[l][[h + 16, h]]
        return _differs(c, redo(mats=mats))
    for d in (8, 16):
        if c.in_dim > d:
            ks = sorted({0, 5, c.in_dim - d - 1}) if c.B >= 16 else range(c.in_dim - d)
            assert need(swapped_x(k, d) for k in ks), f"discrimination: input columns k and k + {d} swapped change nothing"
    probed = range(c.nhm + 2) if c.nhm <= 3 else (0, c.nhm // 2, c.nhm, c.nhm + 1)  # (deep nets: both ends and the middle)
    if c.hidden >= 32:
        for l in probed[:-1]:  # hidden units h and h + 16 of layer l: rows of the matrix that produces them
            hs = sorted({0, 7, c.hidden - 17}) if c.B >= 16 else range(c.hidden - 16)
            assert need(swapped_units(l, h) for h in hs), f"discrimination: hidden units h and h + 16 of layer {l} swapped change nothing"
    for l in probed:  # one non-empty 16x16 tile of every matrix zeroed
        W = c.mats[l]
        rows = c.out_cols if l == c.nhm + 1 else W.shape[0]
        tiles = [(i, j) for i in range(0, rows, 16) for j in range(0, W.shape[1], 16) if np.any(W[i:i + 16, j:j + 16])]
        def zeroed(i, j):
            mats = list(c.mats)
            mats[l] = W.copy()
            mats[l][i:i + 16, j:j + 16] = 0.0
            return _differs(c, redo(mats=mats))
        probe = [tiles[r.integers(len(tiles))]] if c.B >= 16 else tiles
        assert need(zeroed(i, j) for i, j in probe), f"discrimination: a tile of matrix {l} zeroed changes nothing ({probe[0]})"


@functools.lru_cache(maxsize=None)
def get_case(in_dim, hidden, nhm, B, act=ACT_RELU, out_cols=16):
    """The problem the GPU tests use for a shape: built once, conditions asserted on every build."""
    for seed in range(8):  # (a single-row batch fails "every tile counts" for one draw in a few hundred: next seed)
        c = build_case(in_dim, hidden, nhm, B, act, out_cols, seed=seed)
        try:
            check_conditions(c)
            return c
        except AssertionError:
            if seed == 7:
                raise


# ------------------------------------------------------------------------------------------------ lnh_mlp_wgrad alone
class WgradCase:
    """G [P, 256], A [P, 256] in {-2 .. 2}; the problem (M, N) is their first M / N columns, so one product serves all 256."""

    def __init__(self, B, seed=0):
        self.B, self.P = B, min(B, PERIOD)
        self.idx = np.arange(B) % self.P
        self.cnt = np.bincount(self.idx, minlength=self.P).astype(np.float64)
        r = np.random.default_rng([B, seed])
        self.G = r.integers(-2, 3, size=(self.P, 256)).astype(np.float64)
        self.A = r.integers(-2, 3, size=(self.P, 256)).astype(np.float64)
        for t in (self.G, self.A):  # every row counts at every width: a nonzero among its first 16 columns
            dead = ~np.any(t[:, :16] != 0, axis=1)
            t[dead, 0] = 1.0
        self.dW = (self.G * self.cnt[:, None]).T @ self.A

    def check_conditions(self, shapes):
        assert np.all(np.any(self.G[:, :16] != 0, axis=1)) and np.all(np.any(self.A[:, :16] != 0, axis=1)), "every batch row counts"
        bound = (np.abs(self.G) * self.cnt[:, None]).T @ np.abs(self.A)
        assert bound.max() < SUM_LIMIT, f"dW sum bound: {bound.max()} >= 2^24"
        for M, N in shapes:
            d = self.dW[:M, :N]
            assert np.all(np.abs(d).reshape(M // 16, 16, N // 16, 16).max(axis=(1, 3)) > 0), f"every tile counts: ({M}, {N})"
            for keep in (self.B - 1, (self.B - 1) // 16 * 16):  # a dropped last row / last 16-row tile
                cnt = np.bincount(self.idx[:keep], minlength=self.P).astype(np.float64)
                assert not np.array_equal((self.G[:, :M] * cnt[:, None]).T @ self.A[:, :N], d), "discrimination: dropped rows"
            if self.B > 1:  # the row behind the batch (what a tail tile would read one row too far) must change the sum
                assert np.any(np.outer(self.G[0, :M], self.A[0, :N]) != 0)


@functools.lru_cache(maxsize=None)
def get_wgrad_case(B):
    c = WgradCase(B)
    shapes = [(M, N) for M in WGRAD_DIMS for N in WGRAD_DIMS] if B == WGRAD_B else WGRAD_EDGE_SHAPES
    c.check_conditions(shapes)
    return c
