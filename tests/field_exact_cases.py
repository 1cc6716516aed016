"""Integer-valued known-answer problems for the fused LiDAR-field kernels: the sigma net on level-major features with a strided
destination (lnh_density_mlp_*), the colour head over merged and ragged samples (csrc/lidar_color.hip) and the direction-term
glue (lnh_lidar_dir_term*), with their exact answers.  TEST INFRASTRUCTURE ONLY (no GPU); built on tests/mlp_exact_cases.py.

Sigma net: the problems of `mlp_exact_cases.get_case(32, 64, 0, B)` with a layout ([16, B, 2] level-major features) and a
destination map (point p = r * T_cur + j -> row r * T_tot + slot_off + j).

Colour head: x [rows, 16] in {-1 .. 2} (column 0, the density pre-activation, in {-1 .. 2} with a few rows at +-16), cdir
[N, 64] small integers, W0g three +-1 per row in columns 1 .. 15 (column 0 zero), W1 a permutation plus one +-1 per row, W2
four +-1 in each of rows 0 and 1.  h0, h1 and o are integers.  Weights are exactly 0, 2^-20 (below the 1e-4 mask) or 2^-10 k,
k in 1 .. 4 (above it).  The sigmoid and the exponential of the backward are not integer-valued, so the incoming gradients are
PRE-COMPENSATED: a probe (an active sample with |o_0| <= 2 and |o_1| <= 2) gets g_rgb = fl32(t / (s (1 - s))), s = sigmoid(o)
in float64, t a signed integer in 1 .. 4, and every sample gets g_sigma = fl32(t' / exp(clamp(x_0, -15, 15))): the first
16-bit values the backward forms, g_rgb r (1 - r) and g_sigma exp(.), then differ from t and t' by far less than half a 16-bit
spacing and round to them, and everything downstream (g_h16, dW2, dW1, dW0g, S) is an integer with one right value in any
summation order.  Every other active sample gets g_rgb = 0.  Masked samples with |o| <= 2 ("decoys") get a compensated g_rgb as
well: a kernel that lets one through its mask changes an answer; a right kernel ignores it.

cdir takes one of N_CLASS vectors (ray n has class n % N_CLASS, so neighbouring rays differ) and the rows of x come from a pool
per class whose outputs are known, which lets the generator put a probe at a chosen merged position.  The expected tensors are
NOT read off the pools: `ColorCase.expected()` evaluates the head in float64 on the arrays the kernel is given.
"""
import functools

import numpy as np

import mlp_exact_cases as mc

VALUE_LIMIT, SUM_LIMIT = mc.VALUE_LIMIT, mc.SUM_LIMIT
THRESH = 1e-4                     # the colour mask of the renderer
W_BELOW, W_UNIT = 2.0 ** -20, 2.0 ** -10
PROBE_O = 2                       # a probe has |o| <= PROBE_O in both outputs
N_CLASS, POOL = 31, 2048
S_PERTURB = 2.0 ** -17            # relative perturbation of the sigmoid the compensation must survive
RGB_BOUND_ULPS = 8                # |rgb - sigmoid(o)| <= (|o| + 8) 2^-24 sigmoid(o)  (derived in test_field_exact_gpu.py)

# ------------------------------------------------------------------------------------------------ the shapes of the GPU file
SIGMA_SHAPES = [(1, 1, 1, 0), (3, 5, 9, 2), (1, 127, 127, 0), (2, 64, 80, 16), (5, 129, 200, 71)]   # (N, T_cur, T_tot, off)
SIGMA_FWD_STRIDE = (2049, 128, 130, 1)     # > 2048 workgroups x 128 points
SIGMA_BWD_STRIDE = (65, 1009, 1009, 0)     # > 256 workgroups x 256 points
COLOR_FWD_SHAPES = [(1, 1), (3, 21), (5, 64)]
COLOR_FWD_STRIDE = (2050, 257)             # > 2048 workgroups x 256 samples; rays tile a period of STRIDE_RAYS rays
STRIDE_RAYS = 7
COLOR_BWD_SHAPES = [(4, 20), (3, 32), (3, 33), (2, 1024), (2, 1025), (2, 2200)]
COLOR_WAVE_SHAPES = [(1027, 40), (2100, 40), (3100, 97)]   # more rays than the 1024 resident waves; (3100, 97): four rays a wave
COMPOSITE_T = (1, 63, 64, 65, 448, 449, 2048)
COMPOSITE_N = 5
RESIDENT_WAVES = 1024                      # 256 workgroups x 4 waves of the colour backward
RAGGED_COUNTS = (0, 1, 31, 32, 33, 1024, 1025, 5, 64, 0, 100, 17)   # entry 10 does not fit the buffers (dropped)
RAGGED_DROPPED = 10
DIR_N, DIR_K = (1, 3, 4, 5, 257), (1, 27, 75, 128)
DIRB_N, DIRB_K = (1, 15, 16, 17, 257, 4099), (1, 27, 75, 128)


def sigmoid(o):
    return 1.0 / (1.0 + np.exp(-np.asarray(o, dtype=np.float64)))


def round16(v, bf16):
    if bf16:
        return mc.mlp_ref.round_bf16(v).astype(np.float64)
    return np.asarray(v).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------ sigma net
class SigmaCase:
    def __init__(self, N, T_cur, T_tot, off):
        self.N, self.T_cur, self.T_tot, self.off = N, T_cur, T_tot, off
        self.B, self.B_all = N * T_cur, N * T_tot
        self.c = mc.get_case(32, 64, 0, self.B)
        p = np.arange(self.B)
        self.rows = (p // T_cur) * T_tot + off + p % T_cur     # destination row of point p

    def check_conditions(self):
        c = self.c
        assert len(np.unique(self.rows)) == self.B and self.rows.max() < self.B_all
        assert np.abs(c.y[:, 0]).max() <= 80, "sigma = exp(y0) must stay a normal fp32 number"
        if self.B > 1:  # the level-major layout differs from the row-major one, the strided rows from the dense ones
            x = c.x[c.idx]
            assert not np.array_equal(x.reshape(self.B, 16, 2).transpose(1, 0, 2).reshape(self.B, 32), x)
        if self.N > 1 and self.T_tot != self.T_cur:
            assert not np.array_equal(self.rows, np.arange(self.B))


@functools.lru_cache(maxsize=None)
def get_sigma_case(N, T_cur, T_tot, off):
    s = SigmaCase(N, T_cur, T_tot, off)
    s.check_conditions()
    return s


# ------------------------------------------------------------------------------------------------ colour head
class Head:
    def __init__(self, seed=11):
        r = np.random.default_rng(seed)
        self.W0g = np.zeros((64, 16))
        self.W0g[:, 1:] = mc._sparse_rows(r, 64, 15, 3)
        self.W1 = mc._hidden_matrix(r, 64, "perm+1")
        self.W2 = np.zeros((16, 64))
        self.W2[:2] = mc._sparse_rows(r, 2, 64, 4)
        self.cdir = r.integers(-2, 3, size=(N_CLASS, 64)).astype(np.float64)
        self.pool_x = r.integers(-1, 3, size=(N_CLASS, POOL, 16)).astype(np.float64)
        o = np.stack([self.forward(self.pool_x[k], self.cdir[k][None])[2] for k in range(N_CLASS)])
        quiet = np.abs(o).max(axis=2) <= PROBE_O
        self.quiet = [np.flatnonzero(q) for q in quiet]
        self.loud = [np.flatnonzero(~q) for q in quiet]
        assert min(len(q) for q in self.quiet) >= 32

    def forward(self, x, cd, W1=None):
        h0 = np.maximum(x @ self.W0g.T + cd, 0.0)
        h1 = np.maximum(h0 @ (self.W1 if W1 is None else W1).T, 0.0)
        return h0, h1, h1 @ self.W2[:2].T

    def flat(self):
        return np.concatenate([self.W0g.ravel(), self.W1.ravel(), self.W2.ravel()])


@functools.lru_cache(maxsize=None)
def head():
    return Head()


def _ray_modes(N, T):
    """How many 32-sample spans of ray n hold an active sample: -1 = every sample drawn independently."""
    nsp = (T + 31) // 32
    if N > RESIDENT_WAVES:  # wave w walks rays w, w + 1024, ...: consecutive items of ONE wave cross these rays
        w, q = np.arange(N) % RESIDENT_WAVES, np.arange(N) // RESIDENT_WAVES
        if nsp >= 4:        # 0, 1, 2, 3 active spans in consecutive rays of a walk, in every rotation
            return (w + q) % 4
        # T = 40 (two spans): bit q of w & 7 makes the q-th ray of the walk transparent (first, last, two in a row, all three)
        transparent = ((w & 7) >> q) & 1
        return np.where(transparent == 1, 0, np.array([-1, 1, 2])[(w + q) % 3])
    modes = np.full(N, -1)
    if N >= 3:
        modes[1] = 0        # a ray without any active sample
    if N >= 2:
        modes[N - 1] = -2   # a single active sample
    return modes


class ColorCase:
    """One colour-head problem over a sample list.  Sample m: `ray[m]` (row of cdir and S), `xrow[m]` (row of h16 / g_h16),
    `pos[m]` (row of weights / rgb / g_rgb / g_sigma), `act[m]`.  Dense: m = n T + i, xrow = n T + perm[n, i], pos = m.
    Ragged: the owned rows of the flat buffers, xrow = pos = offset + i, all active."""

    def __init__(self, N, T=None, rays=None, M=None, seed=0):
        H = head()
        self.N, self.T, self.H = N, T, H
        self.ragged = rays is not None
        r = np.random.default_rng([N, T or 0, M or 0, seed])
        forced = []  # (ray-local sample list index) positions that must hold a probe
        if not self.ragged:
            self.rows = N * T
            self.scale = 1.0
            self.perm = np.stack([r.permutation(T) for _ in range(N)])
            ray = np.repeat(np.arange(N), T)
            i = np.tile(np.arange(T), N)
            pos = np.arange(N * T)
            xrow = ray * T + self.perm.ravel()
            modes = _ray_modes(N, T)
            act = np.zeros((N, T), bool)
            must = np.zeros((N, T), bool)
            nsp = (T + 31) // 32
            for n in range(N):
                k = modes[n]
                if k == -1:
                    act[n] = r.random(T) < 0.5
                elif k == -2:
                    j = r.integers(T)
                    act[n, j] = must[n, j] = True
                else:
                    for sp in r.choice(nsp, size=min(k, nsp), replace=False):
                        lo, hi = sp * 32, min(T, sp * 32 + 32)
                        js = r.choice(np.arange(lo, hi), size=min(hi - lo, 1 + r.integers(3)), replace=False)
                        act[n, js] = True
                        must[n, js[0]] = True
            if modes[0] == -1:  # the last valid sample of a partial span, the first sample of the second 1024-sample group
                for j in ([T - 1] if T % 32 else []) + ([1024] if T > 1024 else []) + [0]:
                    act[0, j] = must[0, j] = True
            act, must = act.ravel(), must.ravel()
        else:
            self.rays, self.rows, self.scale = rays, M, 2.0
            ray, i, pos = [], [], []
            for rid, off, cnt in rays:
                if off + cnt > M:
                    continue
                ray += [rid] * cnt
                i += list(range(cnt))
                pos += list(range(off, off + cnt))
            ray, i, pos = np.array(ray), np.array(i), np.array(pos)
            xrow = pos
            act = np.ones(len(pos), bool)
            must = np.zeros(len(pos), bool)
            for rid, off, cnt in rays:
                if off + cnt <= M and cnt:
                    for j in {cnt - 1, 0, 1024 if cnt > 1024 else 0}:
                        must[np.flatnonzero(pos == off + j)] = True
        self.ray, self.i, self.pos, self.xrow, self.act = ray, i, pos, xrow, act
        S = len(pos)
        cls = ray % N_CLASS
        want_quiet = must | (r.random(S) < 0.4)
        u = r.random(S)
        pick = np.zeros(S, np.int64)
        for k in range(N_CLASS):
            for q, pool in ((True, H.quiet[k]), (False, H.loud[k])):
                sel = np.flatnonzero((cls == k) & (want_quiet == q))
                pick[sel] = pool[(u[sel] * len(pool)).astype(np.int64)]
        self.x = np.full((self.rows, 16), np.nan)
        self.x[xrow] = H.pool_x[cls, pick]
        x0 = r.integers(-1, 3, size=S).astype(np.float64)
        x0[r.random(S) < 0.03] = 16.0
        x0[r.random(S) < 0.03] = -16.0
        self.x[xrow, 0] = x0
        self.cdir = H.cdir[np.arange(N) % N_CLASS]
        self.weights = np.full(self.rows, np.nan)
        self.weights[pos] = np.where(act, W_UNIT * r.integers(1, 5, size=S), np.where(r.random(S) < 0.3, 0.0, W_BELOW))
        # ---- the float64 reference of the forward, then the compensated gradients
        self.o = self._forward_all()
        self.quiet = np.abs(self.o).max(axis=1) <= PROBE_O
        assert np.array_equal(self.quiet, want_quiet), "the pools and the reference disagree about a sample"
        self.probe = self.quiet & act
        sgn = lambda n: r.integers(1, 5, size=n) * r.choice([-1, 1], size=n)
        self.t = np.zeros((S, 2))
        self.t[self.quiet] = np.stack([sgn(int(self.quiet.sum())), sgn(int(self.quiet.sum()))], axis=1)
        self.tq = sgn(S).astype(np.float64)
        s = sigmoid(self.o)
        self.g_rgb = np.full((self.rows, 2), np.nan, dtype=np.float32)
        self.g_rgb[pos] = np.where(self.quiet[:, None], self.t / np.where(self.quiet[:, None], s * (1 - s), 1.0), 0.0).astype(np.float32)
        self.g_sigma = np.full(self.rows, np.nan, dtype=np.float32)
        self.g_sigma[pos] = (self.tq / np.exp(np.clip(x0, -15, 15))).astype(np.float32)
        self._exp = None

    # ---- reference
    def _forward_all(self, ray=None, xrow=None, W1=None, sel=None):
        ray, xrow = self.ray if ray is None else ray, self.xrow if xrow is None else xrow
        if sel is not None:
            ray, xrow = ray[sel], xrow[sel]
        o = np.zeros((len(ray), 2))
        for a in range(0, len(ray), 32768):
            b = slice(a, a + 32768)
            o[b] = self.H.forward(self.x[xrow[b]], self.cdir[ray[b]], W1)[2]
        return o

    def by_of(self, m, o=None):
        """d loss / d o of samples m as the kernel forms it: g_rgb s (1 - s), an integer to ~1e-7 on an unmutated problem."""
        s = sigmoid(self.o[m] if o is None else o)
        by = self.g_rgb[self.pos[m]].astype(np.float64) * s * (1 - s)
        near = np.abs(by - np.rint(by)) < 1e-3
        return np.where(near, np.rint(by), by)

    def backward(self, m, by=None, ray=None, xrow=None):
        """Samples m taken as active: (dH1, dH0, dx, h0, h1, x) in float64."""
        ray, xrow = self.ray if ray is None else ray, self.xrow if xrow is None else xrow
        x = self.x[xrow[m]]
        h0, h1, o = self.H.forward(x, self.cdir[ray[m]])
        by = self.by_of(m, o) if by is None else by
        dH1 = (by @ self.H.W2[:2]) * (h1 > 0)
        dH0 = (dH1 @ self.H.W1) * (h0 > 0)
        return dict(by=by, dH1=dH1, dH0=dH0, dx=dH0 @ self.H.W0g, h0=h0, h1=h1, x=x)

    def sums(self, m, mult=None, **kw):
        """Contribution of samples m (taken as active) to dW0g, dW1, dW2 and to the rows of S."""
        b = self.backward(m, **kw)
        w = np.ones(len(m)) if mult is None else mult
        S = np.zeros((self.N, 64))
        np.add.at(S, self.ray[m], b["dH0"] * w[:, None])
        dW2 = np.zeros((16, 64))
        dW2[:2] = (b["by"] * w[:, None]).T @ b["h1"]
        return dict(dW0g=(b["dH0"] * w[:, None]).T @ b["x"], dW1=(b["dH1"] * w[:, None]).T @ b["h0"], dW2=dW2, S=S)

    def expected(self):
        """rgb [rows, 2] (float64 sigmoid; 0 on masked samples; NaN where no sample owns the row), g_h16 [rows, 16] (NaN
        likewise), dW0g, dW1, dW2, S [N, 64]."""
        if self._exp is None:
            m = np.flatnonzero(self.probe)
            b = self.backward(m)
            assert np.array_equal(b["by"], self.t[m]), "the compensated gradient does not come back as its integer"
            gh = np.full((self.rows, 16), np.nan)
            gh[self.xrow] = 0.0
            gh[self.xrow[m]] = b["dx"]
            gh[self.xrow, 0] = self.scale * self.tq
            rgb = np.full((self.rows, 2), np.nan)
            rgb[self.pos] = np.where(self.act[:, None], sigmoid(self.o), 0.0)
            self._exp = dict(self.sums(m), rgb=rgb, g_h16=gh, bwd=b)
        return self._exp

    def flat_dW(self):
        e = self.expected()
        return np.concatenate([e["dW0g"].ravel(), e["dW1"].ravel(), e["dW2"].ravel()])

    # ---- where the probes lie
    def position_classes(self):
        """name -> does a probe (or a ray pattern) of this class occur in the problem."""
        out = {}
        pr, i, ray = self.probe, self.i, self.ray
        cnt = np.bincount(ray, minlength=self.N) if self.ragged else np.full(self.N, self.T)
        T_of = cnt[ray]
        out["last valid sample of a partial span"] = bool(np.any(pr & (i == T_of - 1) & (T_of % 32 != 0)))
        out["first sample of the second group"] = bool(np.any(pr & (i == 1024)))
        nact = np.bincount(ray, weights=self.act, minlength=self.N)
        npr = np.bincount(ray, weights=pr, minlength=self.N)
        out["only active sample of a ray"] = bool(np.any((nact == 1) & (npr == 1)))
        out["ray without an active sample"] = bool(np.any(nact == 0))
        if not self.ragged:
            spans = np.zeros((self.N, (self.T + 31) // 32), bool)
            spans[ray[self.act], i[self.act] // 32] = True
            ns = spans.sum(axis=1)
            walks = [ns[w::RESIDENT_WAVES] for w in range(min(self.N, RESIDENT_WAVES))]
            out["consecutive rays with 0, 1, 2, 3 active spans"] = any(
                any(np.array_equal(v[a:a + 4], [0, 1, 2, 3]) for a in range(len(v) - 3)) for v in walks)
            out["transparent ray first in a walk"] = any(len(v) > 1 and v[0] == 0 and v[1] > 0 for v in walks)
            out["transparent ray last in a walk"] = any(len(v) > 1 and v[-1] == 0 and v[-2] > 0 for v in walks)
            out["two transparent rays in a row"] = any(len(v) > 2 and np.any((v[:-1] == 0) & (v[1:] == 0)) and np.any(v > 0) for v in walks)
        return out


def required_classes(c):
    """The position classes a problem must hold BY CONSTRUCTION (tests/test_field_exact_cpu.py asserts them)."""
    if c.ragged:
        return ["last valid sample of a partial span", "first sample of the second group", "only active sample of a ray",
                "ray without an active sample"]
    need = []
    if c.N > RESIDENT_WAVES:
        need += ["consecutive rays with 0, 1, 2, 3 active spans"] if c.T > 96 else \
            ["transparent ray first in a walk", "transparent ray last in a walk"] + \
            (["two transparent rays in a row"] if c.N > 2 * RESIDENT_WAVES else [])   # (needs walks of three rays)
        return need + ["ray without an active sample"]
    if c.T % 32:
        need.append("last valid sample of a partial span")
    if c.T > 1024:
        need.append("first sample of the second group")
    if c.N >= 2:
        need.append("only active sample of a ray")
    if c.N >= 3:
        need.append("ray without an active sample")
    return need


def check_conditions(c, backward=True):
    """The conditions of an exact colour-head test, asserted on the reference alone."""
    H = c.H
    own = ~np.isnan(c.x[:, 0])
    for name, t in dict(x=c.x[own], cdir=c.cdir, W0g=H.W0g, W1=H.W1, W2=H.W2, o=c.o).items():
        assert np.all(np.abs(t) <= VALUE_LIMIT), f"exactness: |{name}| reaches {np.abs(t).max()}"
        assert np.array_equal(round16(t, True), t) and np.array_equal(round16(t, False), t), f"exactness: {name} is not 16-bit"
    assert not np.any(H.W0g[:, 0]) and not np.any(H.W2[2:])
    for W in (H.W0g, H.W1, H.W2[:2]):
        assert len(np.unique(W, axis=0)) == len(W), "two equal units"
    w = c.weights[c.pos]
    assert np.all((w == 0) | (w == W_BELOW) | (w >= W_UNIT)) and np.array_equal(w > THRESH, c.act)
    assert np.all((w > 8 * THRESH) | (w < THRESH / 8)), "a weight within a factor 8 of the mask threshold"
    for a in range(0, len(c.pos), 32768):   # hidden layers of every sample the kernels evaluate
        b = slice(a, a + 32768)
        h0, h1, _ = H.forward(c.x[c.xrow[b]], c.cdir[c.ray[b]])
        assert max(h0.max(), h1.max()) <= VALUE_LIMIT
    if not backward:
        return
    e = c.expected()
    b = e["bwd"]
    for name in ("by", "dH1", "dH0", "dx"):
        assert np.all(np.abs(b[name]) <= VALUE_LIMIT) and np.array_equal(b[name], np.rint(b[name])), f"exactness: {name}"
    assert np.abs(c.scale * c.tq).max() <= VALUE_LIMIT
    bounds = [np.abs(b["dH0"]).T @ np.abs(b["x"]), np.abs(b["dH1"]).T @ np.abs(b["h0"]), np.abs(b["by"]).T @ np.abs(b["h1"])]
    assert max(v.max() for v in bounds) < SUM_LIMIT and np.abs(b["dH0"]).sum(axis=0).max() < SUM_LIMIT, "sum bound"
    # ---- the compensation: s perturbed by a relative +-2^-17 still rounds to t, in fp16 and in bf16; the exponential too
    m = np.flatnonzero(c.quiet)
    s = sigmoid(c.o[m])
    g = c.g_rgb[c.pos[m]].astype(np.float64)
    for eps in (-S_PERTURB, 0.0, S_PERTURB):
        sp = s * (1 + eps)
        for bf in (False, True):
            assert np.array_equal(round16(g * sp * (1 - sp), bf), c.t[m]), "compensation: a perturbed product leaves its integer"
    x0 = c.x[c.xrow, 0]
    assert set(np.unique(x0)) <= {-16.0, -1.0, 0.0, 1.0, 2.0, 16.0}
    for eps in (-S_PERTURB, 0.0, S_PERTURB):
        p = c.g_sigma[c.pos].astype(np.float64) * np.exp(np.clip(x0, -15, 15)) * (1 + eps)
        for bf in (False, True):
            assert np.array_equal(round16(p, bf), c.tq), "compensation: g_sigma exp(.) leaves its integer"
    # ---- no unit dead: every hidden unit fires on a probe and rests on one; every unit W2 (and through it W1) reaches gets a
    #      gradient.  (Problems with few probes cannot hold all of this; the weights are the same in every problem, and
    #      tests/test_field_exact_cpu.py asserts that the larger problems do.)
    if len(c.probe.nonzero()[0]) >= 200:
        for name in ("h0", "h1"):
            assert np.all(np.any(b[name] > 0, axis=0)) and np.all(np.any(b[name] == 0, axis=0)), f"a dead unit in {name}"
            assert len(np.unique(b[name].T, axis=0)) == 64, f"two equal units in {name}"
        r1 = np.any(H.W2[:2] != 0, axis=0)
        r0 = np.any(H.W1[r1] != 0, axis=0)
        assert np.all(np.any(b["dH1"][:, r1] != 0, axis=0)) and np.all(np.any(b["dH0"][:, r0] != 0, axis=0)), "a unit without gradient"
    have = c.position_classes()
    for name in required_classes(c):
        assert have[name], f"position class missing: {name}"


def check_discrimination(c):
    """Each classic mistake, applied to the reference, must change at least one expected tensor."""
    e = c.expected()
    sel = np.arange(min(len(c.pos), 4096))
    probes = np.flatnonzero(c.probe)
    assert len(probes) >= 1

    def changes_sums(m, what, mult=None):
        d = c.sums(np.asarray(m), mult=mult)
        assert all(np.any(d[k] != 0) for k in ("dW0g", "dW1", "dW2") if np.any(e[k])) and np.any(d["dW2"] != 0), \
            f"discrimination: {what} leaves a weight gradient unchanged"
    # a dropped / duplicated active sample: the first and the last probe
    for m in {probes[0], probes[-1]}:
        changes_sums([m], "a dropped or duplicated probe")
    # a sample masked on the wrong side: a decoy let in; the smallest active weights masked out
    decoys = np.flatnonzero(c.quiet & ~c.act)
    if not c.ragged:
        assert len(decoys) or c.T == 1, "no masked sample carries a gradient"
        if len(decoys):
            changes_sums(decoys, "masked samples let in")
            assert np.any(sigmoid(c.o[decoys]) != 0)
        low = np.flatnonzero(c.probe & (c.weights[c.pos] == W_UNIT))
        if len(low):
            changes_sums(low, "active samples of the smallest weight masked out")
    # the neighbour ray's cdir; (ragged) the table's row taken for the ray index
    if c.N > 1:
        nb = (c.ray + 1) % c.N
        assert not np.array_equal(c._forward_all(ray=nb, sel=sel), c.o[sel]), "discrimination: the neighbour ray's cdir"
    if c.ragged:
        row_of_id = np.zeros(c.N, np.int64)
        row_of_id[c.rays[:, 0]] = np.arange(c.N)
        assert not np.array_equal(c._forward_all(ray=row_of_id[c.ray], sel=sel), c.o[sel]), "discrimination: table row for ray id"
        S2 = np.zeros_like(e["S"])
        S2[row_of_id] = e["S"]
        assert not np.array_equal(S2, e["S"]), "discrimination: S indexed by the table row"
    elif c.T > 2:
        for what, p2 in (("ignored", np.tile(np.arange(c.T), (c.N, 1))), ("inverted", np.argsort(c.perm, axis=1))):
            xr = (np.repeat(np.arange(c.N), c.T) * c.T + p2.ravel())
            assert not np.array_equal(c._forward_all(xrow=xr, sel=sel), c.o[sel]), f"discrimination: perm {what}"
            assert not np.array_equal(xr, c.xrow)
    # the last partial span dropped
    part = np.flatnonzero(c.probe & (c.i >= (np.bincount(c.ray, minlength=c.N)[c.ray] // 32) * 32)) if c.ragged else \
        np.flatnonzero(c.probe & (c.i >= c.T // 32 * 32))
    if "last valid sample of a partial span" in required_classes(c):
        changes_sums(part, "the last partial span dropped")
    # a tail row >= rows let in: the rows behind every input are NaN
    assert np.isnan(np.full((1, 16), np.nan) @ c.H.W0g.T).all()
    # W1 transposed
    assert not np.array_equal(c._forward_all(W1=np.ascontiguousarray(c.H.W1.T), sel=sel), c.o[sel]), "discrimination: W1 transposed"
    # a ray without active spans left out of S: its row of S is zero, not the sentinel, and such a ray exists
    if "ray without an active sample" in required_classes(c):
        nact = np.bincount(c.ray, weights=c.act, minlength=c.N)
        assert np.any(nact == 0) and not np.any(e["S"][nact == 0])


@functools.lru_cache(maxsize=None)
def get_color_case(N, T, backward=True):
    for seed in range(8):
        c = ColorCase(N, T, seed=seed)
        try:
            check_conditions(c, backward)
            return c
        except AssertionError:
            if seed == 7:
                raise


def ragged_table():
    """rays [N, 3] (id, offset, count) and M: ids a permutation, offsets handed out in a shuffled order with gaps of rows
    nobody owns, entry RAGGED_DROPPED reaching past M."""
    r = np.random.default_rng(77)
    N = len(RAGGED_COUNTS)
    ids = r.permutation(N)
    rays = np.zeros((N, 3), np.int64)
    acc = 3
    for e in r.permutation(N):
        if e == RAGGED_DROPPED:
            continue
        rays[e] = (ids[e], acc, RAGGED_COUNTS[e])
        acc += RAGGED_COUNTS[e] + int(r.integers(0, 6))
    M = acc + 50
    rays[RAGGED_DROPPED] = (ids[RAGGED_DROPPED], M - 50, RAGGED_COUNTS[RAGGED_DROPPED])
    return rays, M


@functools.lru_cache(maxsize=None)
def get_ragged_case():
    rays, M = ragged_table()
    for seed in range(8):
        c = ColorCase(len(rays), None, rays=rays, M=M, seed=seed)
        try:
            check_conditions(c)
            assert rays[RAGGED_DROPPED, 1] + rays[RAGGED_DROPPED, 2] > M and np.isnan(c.x[:, 0]).sum() > 50
            return c
        except AssertionError:
            if seed == 7:
                raise


class TiledForward:
    """The periodic forward problem: ray n of (N, T) is ray n % STRIDE_RAYS of a (STRIDE_RAYS, T) problem."""

    def __init__(self, N, T):
        self.N, self.T, self.p = N, T, get_color_case(STRIDE_RAYS, T, False)
        self.reps = -(-N // STRIDE_RAYS)

    def tile(self, a):
        """[STRIDE_RAYS * T, ...] -> [N * T, ...]"""
        a = a.reshape((STRIDE_RAYS, self.T) + a.shape[1:])
        return np.concatenate([a] * self.reps)[:self.N].reshape((self.N * self.T,) + a.shape[2:])


# ------------------------------------------------------------------------------------------------ composite forward
class CompositeCase:
    """The inputs of lnh_lidar_color_composite_forward on top of a colour problem: sorted z with a constant step, sigma_pt 0
    or `SIGMA` at up to 9 merged positions of a ray, so every float64 weight is exactly 0 or >= 2^-9 > 1e-3."""
    SIGMA, STEP = 64.0, 2.0 ** -6  # alpha = 1 - exp(-1): weights (1 - 1/e) e^-k >= 0.63 e^-8 > ... see check below

    def __init__(self, N, T):
        self.c = c = get_color_case(N, T, False)
        r = np.random.default_rng([N, T, 5])
        self.N, self.T = N, T
        self.z = np.tile(0.25 + self.STEP * np.arange(T), (N, 1))
        self.sd = np.full(N, self.STEP)
        on = np.zeros((N, T), bool)
        for n in range(N):
            if n != 1 or N == 1:
                on[n, r.choice(T, size=min(T, int(r.integers(1, 6))), replace=False)] = True
        self.on = on
        sig_m = np.where(on, self.SIGMA, 0.0)
        self.sigma_pt = np.zeros((N, T))
        np.put_along_axis(self.sigma_pt, c.perm, sig_m, axis=1)
        self.sigma_m = sig_m
        alpha = 1.0 - np.exp(-self.STEP * sig_m)
        trans = np.cumprod(np.concatenate([np.ones((N, 1)), 1.0 - alpha + 1e-15], axis=1), axis=1)[:, :-1]
        self.w = alpha * trans
        assert np.all((self.w == 0) | (self.w >= 1e-3)) and np.array_equal(self.w > 0, on)
        self.rgb = np.where(on.reshape(-1, 1), sigmoid(c.o), 0.0)
        self.o = c.o


@functools.lru_cache(maxsize=None)
def get_composite_case(T):
    return CompositeCase(COMPOSITE_N, T)


# ------------------------------------------------------------------------------------------------ direction-term glue
class DirCase:
    """Integer dir_features [N, K] and w0 [64, ldw] (columns >= K NaN: they belong to other terms and are not read)."""

    def __init__(self, N, K, ldw):
        r = np.random.default_rng([N, K, ldw])
        self.N, self.K, self.ldw = N, K, ldw
        self.f = r.integers(-2, 3, size=(N, K)).astype(np.float64)
        self.w0 = np.full((64, ldw), np.nan)
        self.w0[:, :K] = r.integers(-2, 3, size=(64, K))
        self.cdir = self.f @ self.w0[:, :K].T
        self.S = r.integers(-2, 3, size=(N, 64)).astype(np.float64)
        for t in (self.f, self.S):  # every ray counts: a nonzero in its first column
            t[t[:, 0] == 0, 0] = 1.0
        self.cdir = self.f @ self.w0[:, :K].T
        self.gw0 = self.S.T @ self.f
        self.w0g = r.integers(-9, 10, size=(64, 16)).astype(np.float64)
        assert np.abs(self.cdir).max() < SUM_LIMIT and (np.abs(self.S).T @ np.abs(self.f)).max() < SUM_LIMIT
        if N > 1:  # a dropped last ray changes the sum (of some element)
            assert np.any(np.outer(self.S[-1], self.f[-1]) != 0)


@functools.lru_cache(maxsize=None)
def get_dir_case(N, K, ldw):
    return DirCase(N, K, ldw)
