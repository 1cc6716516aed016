"""Problems and the float64 reference of tests/test_loss_exact_gpu.py (NumPy only; the conditions are asserted without a GPU by
tests/test_loss_exact_cpu.py): the three loss kernels of csrc/lidar_glue.hip — lnh_lidar_loss, lnh_lidar_loss_patch and
lnh_lidar_loss_ex — which emit the loss and the two cotangents the whole backward pass starts from.

`reference` restates the contract of include/lidarnerf_hip.h in float64 with explicit loops over patches, pixels and stencil
taps (a plain cross-correlation with the two 3 x 3 Sobel matrices and zero padding; every derivative scattered tap by tap).  It
calls neither lidarnerf.nerf.loss nor anything shaped like the kernel's recomputation scheme.  Beside the loss and the two
gradients it returns, for every output element, A = the sum of the absolute values of the addends that form it, which the
bounds of tier B are stated in.

INPUTS ARE DYADIC.  gr is 0 or 1, scale, huber_delta and every alpha are powers of two, depths are scale * k * 2^-12 (2^-10 in
tier A) with small integer k, image values multiples of 2^-8.  Then depth * gr / scale, every neighbour difference, every Sobel
response and so every mask decision is exact in float32 and the same number in float64: a mask cannot flip between kernel
and reference.  `check_conditions` asserts this for every case.

TIER A — one right float32 value in any order.  Criteria L1, MSE, HUBER with SPATIAL and TV, every mean over a power of two of
elements (per-ray terms: N a power of two; Sobel: any patch shape with N a power of two; without Sobel 2 x 2 only).  The alphas
are chosen per slot so that every loss term is a multiple of one quantum q with sum |terms| < 2^24 q: every partial sum in any
order is exact, and the same holds for the addends of every gradient element.  Compared with torch.equal.

TIER B — everything else (element counts that are no powers of two, BCE, GRAD_NORM_SMOOTH, COS): each output element within
K * 2^-24 * A of the float64 value, K counted on the longest chain of roundings of the kernel text (`k_loss`, `k_gdepth`,
`k_gimage`; DESIGN.md, "Exact tests of the loss kernels").
"""
import functools
import math

import numpy as np

F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32
L1, MSE, HUBER, BCE, COS = range(5)                # LNH_LOSS_*
SOBEL, GRAD, GN, SPATIAL, TV = 1, 2, 4, 8, 16       # LNH_LOSS_* flags
CRIT_NAMES = {L1: "l1", MSE: "mse", HUBER: "huber", BCE: "bce", COS: "cos"}
DEFAULT_CRIT = (L1, MSE, MSE, L1)
WG, SUM_WG = 256, 1024              # rays per workgroup of k_lidar_loss_ex; threads of the single-workgroup kernels
THRESH = float(F(0.01))             # the kernels (and float32 torch) compare float32 gradients with 0.01f
COS_EPS = 1e-8
KX = ((-1.0, 0.0, 1.0), (-2.0, 0.0, 2.0), (-1.0, 0.0, 1.0))
KY = ((-1.0, -2.0, -1.0), (0.0, 0.0, 0.0), (1.0, 2.0, 1.0))
ALPHA_NAMES = ("a_d", "a_r", "a_i", "a_g", "a_gn", "a_sp", "a_tv")
FIXED_ALPHAS = dict(a_d=8.0, a_r=1.0, a_i=2.0, a_g=16.0, a_gn=0.5, a_sp=0.25, a_tv=2.0)


class Case:
    def __init__(self, name, px, py, crit, flags, scale, delta, alphas, depth, image, gt, lattice, f32_threshold=False):
        self.name, self.px, self.py, self.crit, self.flags = name, int(px), int(py), tuple(crit), int(flags)
        self.scale, self.delta, self.alphas = float(scale), float(delta), dict(alphas)
        self.depth, self.image, self.gt = (np.ascontiguousarray(a, dtype=np.float64) for a in (depth, image, gt))
        self.N = self.depth.shape[0]
        self.lattice = lattice              # metres lattice of the depths (None: float32 numbers off the lattice, tie cases)
        self.f32_threshold = f32_threshold  # holds a truth gradient in [fl(0.01f), 0.01): float64 torch masks it differently
        self.closed = {}                    # closed-form expectations: output name -> (ray indices, float64 values)
        assert self.image.shape == (self.N, 2) and self.gt.shape == (self.N, 3)

    @property
    def S(self):
        return self.px * self.py

    @property
    def sobel(self):
        return bool(self.flags & SOBEL)

    @property
    def tier(self):
        return "A" if is_tier_a(self) else "B"

    @property
    def is_default(self):
        """The loss lnh_lidar_loss (px = 1) / lnh_lidar_loss_patch (px > 1) state."""
        return self.crit[:3] == DEFAULT_CRIT[:3] and (self.px == 1 or (self.crit[3] == L1 and self.flags == GRAD))

    def entries(self):
        return ("ex",) + ((("ray",) if self.px == 1 else ("patch",)) if self.is_default else ())

    def replace_depth(self, ray, value):
        c = Case(self.name + "+changed", self.px, self.py, self.crit, self.flags, self.scale, self.delta, self.alphas,
                 self.depth.copy(), self.image, self.gt, self.lattice, self.f32_threshold)
        c.depth[ray] = value
        return c


def _pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def counts(c):
    """Element counts of the means: rays, x tensor, y tensor, gradient term."""
    if c.px <= 1:
        return c.N, 0, 0, 0
    P, sob = c.N // c.S, 1 if c.sobel else 0
    nx, ny = P * c.px * (c.py - 1 + sob), P * (c.px - 1 + sob) * c.py
    return c.N, nx, ny, (P if c.crit[3] == COS else nx)


def is_tier_a(c):
    if c.lattice is None or any(k in (BCE, COS) for k in c.crit[:3]) or not _pow2(max(c.N, 1)):
        return False
    if c.px <= 1:
        return True
    if c.crit[3] in (BCE, COS) or c.flags & GN:
        return False
    return all(_pow2(n) for n in counts(c)[1:3])


# ================================================================================================ the float64 reference
def _crit(c, x, y, delta):
    """Criterion `c` (reduction 'none') on float64 arrays: value, d value / d x, and the sums of |addends| of both."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = x - y
    if c == L1:
        return np.abs(d), np.sign(d), np.abs(d), np.abs(np.sign(d))
    if c == MSE:
        return d * d, 2.0 * d, d * d, np.abs(2.0 * d)
    if c == HUBER:   # torch.nn.HuberLoss: |d| < delta ? d^2 / 2 : delta (|d| - delta / 2)
        a = np.abs(d)
        quad = a < delta
        v = np.where(quad, 0.5 * d * d, delta * (a - 0.5 * delta))
        g = np.clip(d, -delta, delta)
        return v, g, np.where(quad, v, delta * (a + 0.5 * delta)), np.abs(g)
    assert c == BCE  # BCEWithLogitsLoss: (1 - y) x - log sigmoid(x), log sigmoid(x) = min(x, 0) - log1p(e^-|x|)
    with np.errstate(over="ignore"):
        lg = np.log1p(np.exp(-np.abs(x)))
        s = 1.0 / (1.0 + np.exp(-x))
    v = (1.0 - y) * x - (np.minimum(x, 0.0) - lg)
    return v, s - y, np.abs((1.0 - y) * x) + np.abs(np.minimum(x, 0.0)) + lg, s + np.abs(y)


class Ref:
    """loss, g_depth [N], g_image [N, 2]; A_* the sums of |addends|; `terms` every loss term with its slot tag; `q_*` the
    exponent of the lowest set bit over the addends of each gradient element (tier A's lattice check)."""


def _lsb(x):
    """Exponent of the lowest set bit of every float64 in x (a large number for 0)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    tz = np.where(mi == 0, 0, np.frexp(low.astype(np.float64))[1] - 1)
    return np.where(mi == 0, 4096, e - 53 + tz)


def reference(c, alphas=None):
    al = c.alphas if alphas is None else alphas
    N, px, py, S, scale = c.N, c.px, c.py, c.S, c.scale
    _, nx, ny, ng = counts(c)
    gr = c.gt[:, 0]
    gi, gd = c.gt[:, 1] * gr, c.gt[:, 2] * gr
    pr, pi, pd = c.image[:, 0], c.image[:, 1] * gr, c.depth * gr
    r = Ref()
    tags, vals, As = [], [], []          # loss terms
    gdn, gdv, gda = [], [], []           # addends of g_depth: ray, value, |addend| measure
    r.g_image, r.A_gimage = np.zeros((N, 2)), np.zeros((N, 2))
    if N:
        for tag, a, k, x, y in (("d", al["a_d"], c.crit[0], pd, gd), ("r", al["a_r"], c.crit[1], pr, gr),
                                ("i", al["a_i"], c.crit[2], pi, gi)):
            v, g, Av, Ag = _crit(k, x, y, c.delta)
            tags += [tag] * N
            vals.append(a * v / N)
            As.append(a * Av / N)
            if tag == "d":
                gdn.append(np.arange(N))
                gdv.append(a * g * gr / N)
                gda.append(a * Ag * gr / N)
            else:
                col = 0 if tag == "r" else 1
                w = 1.0 if tag == "r" else gr
                r.g_image[:, col], r.A_gimage[:, col] = a * g * w / N, a * Ag * w / N
    vals, As = [np.concatenate(vals)] if vals else [], [np.concatenate(As)] if As else []
    pt, pv, pa, an, av, aa = [], [], [], [], [], []   # patch terms / patch addends of g_depth (python lists)
    r.mask_on, r.mask_all = 0, 0
    if px > 1:
        cos = bool(c.flags & GRAD) and c.crit[3] == COS
        for b in range(0, N, S):
            pred = [[c.depth[b + i * py + j] * gr[b + i * py + j] / scale for j in range(py)] for i in range(px)]
            truth = [[c.gt[b + i * py + j, 2] * gr[b + i * py + j] / scale for j in range(py)] for i in range(px)]

            def at(v, i, j):
                return v[i][j] if 0 <= i < px and 0 <= j < py else 0.0

            def smooth(pg, count):
                """Smoothness terms of one element, (tag, value), and the addends of d loss / d pg."""
                dx, sg, t, parts = abs(pg), float(np.sign(pg)), [], []
                if c.flags & GN:
                    e = math.exp(-dx)
                    t.append(("gn", al["a_gn"] * e / count))
                    parts.append(-al["a_gn"] * e / count * sg)
                if c.flags & SPATIAL:
                    t.append(("sp", al["a_sp"] * dx * dx / count))
                    parts.append(al["a_sp"] * 2.0 * dx / count * sg)
                if c.flags & TV:
                    t.append(("tv", al["a_tv"] * dx / count))
                    parts.append(al["a_tv"] / count * sg)
                return t, [(p, abs(p)) for p in parts]

            def scatter(taps, ds, parts):
                for (k, l), w in taps:
                    n = b + k * py + l
                    for p, ap in parts:
                        an.append(n)
                        av.append(p * ds * w * gr[n] / scale)
                        aa.append(ap * abs(ds * w) * gr[n] / scale)

            xs = []  # the x elements of the patch: (taps, s, pg, gg, m)
            for i in range(px):
                for j in range(py if c.sobel else py - 1):
                    if c.sobel:
                        taps = [((i + a, j + e), KX[a + 1][e + 1]) for a in (-1, 0, 1) for e in (-1, 0, 1)
                                if KX[a + 1][e + 1] != 0.0 and 0 <= i + a < px and 0 <= j + e < py]
                        s = sum(w * at(pred, k, l) for (k, l), w in taps)
                        gg = sum(w * at(truth, k, l) for (k, l), w in taps)
                        pg = s
                    else:
                        taps = [((i, j), 1.0), ((i, j + 1), -1.0)]
                        s, gg = pred[i][j] - pred[i][j + 1], truth[i][j] - truth[i][j + 1]
                        pg = abs(s)
                    m = gr[b + i * py + j] if abs(gg) < THRESH else 0.0
                    xs.append((taps, s, pg, gg, m))
                    if c.flags & GRAD and gr[b + i * py + j] > 0:
                        r.mask_all += 1
                        r.mask_on += int(m > 0)
            if cos:
                u = [e[2] * e[4] for e in xs]
                w = [e[3] * e[4] for e in xs]
                uw, uu, ww = sum(p * q for p, q in zip(u, w)), sum(p * p for p in u), sum(q * q for q in w)
                un, wn = math.sqrt(uu), math.sqrt(ww)
                nu, nw = max(un, COS_EPS), max(wn, COS_EPS)
                cs = uw / (nu * nw)
                P = N // S
                pt.append("g")
                pv.append(al["a_g"] * (1.0 - cs) / P)
                pa.append(al["a_g"] * 2.0 / P)       # the addends 1 and cos, cos counted as 1 (its error is absolute)
            for taps, s, pg, gg, m in xs:
                t, parts = smooth(pg, nx)
                if c.flags & GRAD:
                    if cos:
                        p1 = -al["a_g"] / P * (gg * m) / (nu * nw) * m
                        parts.append((p1, abs(p1)))
                        if un > 0.0:
                            p2 = al["a_g"] / P * cs * (pg * m) / (nu * un) * m
                            parts.append((p2, abs(al["a_g"] / P * (pg * m) / (nu * un) * m)))
                    else:
                        v, g, Av, Ag = _crit(c.crit[3], pg * m, gg * m, c.delta)
                        pt.append("g")
                        pv.append(al["a_g"] * float(v) / ng)
                        pa.append(al["a_g"] * float(Av) / ng)
                        parts.append((al["a_g"] * float(g) * m / ng, al["a_g"] * float(Ag) * m / ng))
                for tag, v in t:
                    pt.append(tag)
                    pv.append(v)
                    pa.append(abs(v))
                scatter(taps, 1.0 if c.sobel else float(np.sign(s)), parts)
            for i in range(px if c.sobel else px - 1):   # the y elements: smoothness only
                for j in range(py):
                    if c.sobel:
                        taps = [((i + a, j + e), KY[a + 1][e + 1]) for a in (-1, 0, 1) for e in (-1, 0, 1)
                                if KY[a + 1][e + 1] != 0.0 and 0 <= i + a < px and 0 <= j + e < py]
                        s = sum(w * at(pred, k, l) for (k, l), w in taps)
                        pg = s
                    else:
                        taps = [((i, j), 1.0), ((i + 1, j), -1.0)]
                        s = pred[i][j] - pred[i + 1][j]
                        pg = abs(s)
                    t, parts = smooth(pg, ny)
                    for tag, v in t:
                        pt.append(tag)
                        pv.append(v)
                        pa.append(abs(v))
                    scatter(taps, 1.0 if c.sobel else float(np.sign(s)), parts)
    tags += pt
    vals.append(np.array(pv, dtype=np.float64))
    As.append(np.array(pa, dtype=np.float64))
    r.tags, r.terms, r.term_A = np.array(tags), np.concatenate(vals), np.concatenate(As)
    r.loss, r.A_loss = float(r.terms.sum()), float(r.term_A.sum())
    gdn, gdv, gda = gdn + [np.array(an, dtype=np.int64)], gdv + [np.array(av)], gda + [np.array(aa)]
    idx, v, a = np.concatenate(gdn).astype(np.int64), np.concatenate(gdv), np.concatenate(gda)
    r.g_depth, r.A_gdepth, r.q_gdepth = np.zeros(N), np.zeros(N), np.full(N, 4096)
    np.add.at(r.g_depth, idx, v)
    np.add.at(r.A_gdepth, idx, a)
    np.minimum.at(r.q_gdepth, idx, _lsb(v))
    return r


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """The reference of a registered case; the conditions that make the comparison exact are asserted on the way."""
    c = get_case(name)
    r = reference(c)
    check_conditions(c, r)
    return r


# ================================================================================================ tier B: the bounds
C_VAL = {L1: 0, MSE: 1, HUBER: 3, BCE: 12}   # roundings of a criterion's value
C_GRAD = {L1: 0, MSE: 1, HUBER: 0, BCE: 7}   # ... of its derivative
T_ULP = 4                                    # a transcendental call: 2 ulp = 4 * 2^-24 relative


def _n_x(c):
    return c.px * (c.py if c.sobel else c.py - 1)


def k_loss(c, entry):
    steps = -(-max(c.N, 1) // SUM_WG)
    if entry == "ray":      # a term: two products per MSE term, two adds; one add per stride iteration; the tree; 1 / N and its product
        return 4 + steps + 6 + 15 + 2
    if entry == "patch":    # per iteration: the per-ray chain (6) and the pair (a_g / pairs, its product), two adds to l
        return 6 + 2 + 2 * steps + 6 + 15
    term = max(C_VAL[k] for k in c.crit[:3]) + 5
    if c.px > 1:
        if c.flags & GN:
            term = max(term, T_ULP + 3)
        if c.flags & SPATIAL:
            term = max(term, 4)
        if c.flags & GRAD:
            term = max(term, 2 * _n_x(c) + 9 if c.crit[3] == COS else C_VAL[c.crit[3]] + 3)
    blocks = -(-max(c.N, 1) // WG)
    return term + 11 + 6 + 2 + -(-blocks // SUM_WG) + 6 + 15


def k_gdepth(c, entry):
    if entry == "ray":
        return 3
    if entry == "patch":
        return 8
    k = C_GRAD[c.crit[0]] + 3
    if c.px <= 1:
        return k + 1
    h = 0
    if c.flags & GN:
        h = max(h, T_ULP + 3)
    if c.flags & SPATIAL:
        h = max(h, 3)
    if c.flags & TV:
        h = max(h, 2)
    if c.flags & GRAD:
        h = max(h, 3 * _n_x(c) + 14 if c.crit[3] == COS else C_GRAD[c.crit[3]] + 4)
    return max(k, h + 4) + (12 if c.sobel else 4) + 3


def k_gimage(c, entry):
    return 6 if entry != "ex" else max(C_GRAD[c.crit[1]], C_GRAD[c.crit[2]]) + 5


def ratios(got_loss, got_gd, got_gi, r):
    """error / (2^-24 A) of the loss and the largest over each gradient; an element with A = 0 must be exactly 0."""
    def one(got, want, A):
        got, want, A = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, want, A))
        err = np.abs(got - want)
        err = np.where(np.isfinite(got), err, np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / (U * A))
        return float(q.max()) if q.size else 0.0
    return one(got_loss, r.loss, r.A_loss), one(got_gd, r.g_depth, r.A_gdepth), one(got_gi, r.g_image, r.A_gimage)


# ================================================================================================ data
def _drops(rng, N, S):
    gr = (rng.randint(0, 8, N) > 0).astype(np.float64)
    if N // S >= 4:
        gr[S:2 * S] = 0.0            # one whole dropped patch
    return gr


def _image(rng, N, unit):
    top = int(round(1.0 / unit))
    return rng.randint(0, top + 1, (N, 2)) * unit, rng.randint(0, top + 1, N) * unit


def _patch_fields(rng, P, px, py, sobel, lat, tier_a):
    """Truth and prediction in metres, [P, px, py], on the lattice `lat`.  Sobel: absolute depths below 0.0025 m, so that even
    the border responses (zero padding; weights sum to 4) stay under the 0.01 m mask — except behind a 1 m step in every fifth
    patch (the last one where there are fewer than four).  Without Sobel: a base of whole quarter metres plus small steps, with a step above 0.01 m here and there.
    Tier A keeps every magnitude small (step 2^-6 m, base 0), so that the squares of SPATIAL stay within 24 bits of the sum."""
    if sobel:
        top = int(0.0024 / lat)
        truth = rng.randint(0, top + 1, (P, px, py)).astype(np.float64) * lat
        for p in sorted(set(range(3, P, 5)) | ({P - 1} if P < 4 else set())):
            truth[p, :, (py + 1) // 2:] += 16 * lat if tier_a else 1.0
    else:
        truth = rng.randint(0, 16, (P, 1, 1)) * (0.0 if tier_a else 0.25) + np.cumsum(rng.randint(-3, 4, (P, px, py)), axis=2) * lat
        big = rng.randint(0, 6, (P, px, py)) == 0
        truth = truth + np.cumsum(big, axis=2) * 0.015625
    pred = truth + rng.randint(-3, 4, (P, px, py)) * lat
    return truth, pred


def _auto_alphas(c):
    """Powers of two per slot that put every loss term on the lattice 2^-4 / N (tier A)."""
    ones = {k: 1.0 for k in ALPHA_NAMES}
    r = reference(c, ones)
    out = dict(ones)
    for tag, name in (("d", "a_d"), ("r", "a_r"), ("i", "a_i"), ("g", "a_g"), ("sp", "a_sp"), ("tv", "a_tv")):
        t = r.terms[r.tags == tag]
        t = t[t != 0.0]
        if t.size:
            out[name] = 2.0 ** (-4 - int(math.log2(c.N)) - int(_lsb(t).min()))
    return out


def build(name, N, px, py, crit, flags, seed, tier_a=False, scale=None):
    rng = np.random.RandomState(seed)
    lat = 2.0 ** -10 if tier_a else 2.0 ** -12
    scale = (0.25 if tier_a else 2.0 ** -6) if scale is None else scale
    S = px * py
    gr = _drops(rng, N, S)
    if px > 1:
        truth, pred = _patch_fields(rng, N // S, px, py, bool(flags & SOBEL), lat, tier_a)
    else:
        truth = rng.randint(0, 64, N) * 0.25
        pred = truth + rng.randint(-6, 7, N) * lat
    image, gi = _image(rng, N, 0.25 if tier_a else 2.0 ** -8)
    gt = np.stack([gr, gi, truth.reshape(N) * scale], axis=1) if N else np.zeros((0, 3))
    c = Case(name, px, py, crit, flags, scale, 2.0 * lat, FIXED_ALPHAS, pred.reshape(N) * scale, image, gt, lat)
    if tier_a:
        assert is_tier_a(c), name
        c.alphas = _auto_alphas(c)
    return c


# ================================================================================================ conditions
def check_conditions(c, r=None):
    """What makes the comparison exact; raises AssertionError with the case's name."""
    r = reference(c) if r is None else r
    f32 = lambda a: np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(a, dtype=np.float32).astype(np.float64))
    assert f32(c.depth) and f32(c.image) and f32(c.gt), f"{c.name}: an input is no float32 number"
    assert set(np.unique(c.gt[:, 0])) <= {0.0, 1.0}, f"{c.name}: gr outside {{0, 1}}"
    for v in [c.scale, c.delta] + [c.alphas[k] for k in ALPHA_NAMES]:
        assert v > 0 and math.frexp(v)[0] == 0.5, f"{c.name}: {v} is no power of two"
    if c.lattice is not None:
        k = c.depth / c.scale / c.lattice, c.gt[:, 2] / c.scale / c.lattice
        assert all(np.array_equal(x, np.round(x)) and (np.abs(x) < 2 ** 21).all() for x in k), f"{c.name}: depth off the lattice"
        m = c.image * 256.0, c.gt[:, 1] * 256.0
        assert all(np.array_equal(x, np.round(x)) and (np.abs(x) <= 2 ** 19).all() for x in m), f"{c.name}: image off 2^-8"
        # a Sobel response is a sum of at most 6 lattice numbers with weights 1, 2: below 2^24 lattice units, so exact
        assert 8 * (np.abs(k[0]).max(initial=0) + np.abs(k[1]).max(initial=0)) < 2 ** 24
    if c.px > 1 and c.flags & GRAD:
        if c.sobel:
            assert 2 * r.mask_on >= r.mask_all > 0, f"{c.name}: the mask is on for {r.mask_on} of {r.mask_all} elements"
        else:
            assert r.mask_on > 0, f"{c.name}: the mask is never on"
    if c.tier == "A":
        for what, x in (("loss", r.loss), ("g_depth", r.g_depth), ("g_image", r.g_image)):
            assert f32(x), f"{c.name}: expected {what} is no float32 number"
        q = _lsb(r.terms[r.terms != 0.0]).min() if (r.terms != 0.0).any() else 0
        assert r.A_loss / 2.0 ** int(q) < 2 ** 24, f"{c.name}: sum |terms| needs {math.log2(r.A_loss / 2.0 ** int(q)):.1f} bits"
        on = r.A_gdepth > 0
        assert (r.A_gdepth[on] / 2.0 ** r.q_gdepth[on].astype(np.float64) < 2 ** 24).all(), f"{c.name}: g_depth addends"
        assert (np.abs(r.g_depth[r.g_depth != 0]) >= 2.0 ** -100).all()
    for what, (idx, val) in c.closed.items():
        assert f32(val), f"{c.name}: closed form of {what} is no float32 number"


# ================================================================================================ the cases
SHAPES = ((3, 5, 35), (17, 16, 2), (2, 2, 5), (2, 3, 7), (3, 2, 7), (5, 2, 3), (3, 3, 5), (4, 4, 3), (2, 8, 65))
CONFIGS = (("default", L1, GRAD), ("mse_sobel_spatial", MSE, SOBEL | GRAD | SPATIAL), ("huber_tv", HUBER, GRAD | TV),
           ("bce_sobel_gn", BCE, SOBEL | GRAD | GN), ("cos_all", COS, GRAD | GN | SPATIAL | TV), ("cos_sobel", COS, SOBEL | GRAD),
           ("l1_sobel_all", L1, SOBEL | GRAD | GN | SPATIAL | TV))
_ROT = ((L1, MSE, HUBER), (MSE, HUBER, L1), (HUBER, L1, MSE))
STRADDLE = "3x5x35_"     # patch 17 covers rays 255..269


def _registry():
    reg, seed = {}, 100

    def add(name, fn):
        assert name not in reg
        reg[name] = fn

    for si, (px, py, P) in enumerate(SHAPES):
        for ci, (cname, gc, flags) in enumerate(CONFIGS):
            seed += 1
            per_ray = DEFAULT_CRIT[:3] if ci == 0 else _ROT[(si + ci) % 3]
            if gc == BCE:   # BCE through the per-ray slots too, one slot per shape
                per_ray = tuple(BCE if s == si % 3 else k for s, k in enumerate(per_ray))
            add(f"{px}x{py}x{P}_{cname}", functools.partial(build, f"{px}x{py}x{P}_{cname}", px * py * P, px, py,
                                                          per_ray + (gc,), flags, seed))
    for px, py, P in ((2, 2, 5), (3, 3, 5)):   # smoothness alone, the gradient term off
        add(f"{px}x{py}x{P}_smooth_only", functools.partial(build, f"{px}x{py}x{P}_smooth_only", px * py * P, px, py,
                                                            _ROT[0] + (L1,), SPATIAL | TV | GN, 180 + px))
    # tier A
    for N in (1, 1024):
        for rot in range(3):
            crit = (DEFAULT_CRIT[:3] if rot == 0 else _ROT[rot]) + (L1,)
            add(f"A_ray{N}_{rot}", functools.partial(build, f"A_ray{N}_{rot}", N, 1, 1, crit, 0, 200 + N + rot, True))
    for px, py, P, sob in ((4, 4, 32, SOBEL), (2, 8, 64, SOBEL), (8, 2, 64, SOBEL), (2, 2, 256, 0)):
        for gi, gc in enumerate((L1, MSE, HUBER)):
            add(f"A_{px}x{py}x{P}_{CRIT_NAMES[gc]}", functools.partial(
                build, f"A_{px}x{py}x{P}_{CRIT_NAMES[gc]}", px * py * P, px, py, _ROT[gi] + (gc,), sob | GRAD | SPATIAL | TV,
                300 + 10 * px + gi, True))
    add("A_2x2x256_default", functools.partial(build, "A_2x2x256_default", 1024, 2, 2, DEFAULT_CRIT, GRAD, 390, True))
    # per-ray terms beside the tree sizes of the single-workgroup kernels and in the stride loop of the sum kernel
    for N in (1023, 1025, WG * 1025):
        add(f"ray{N}_default", functools.partial(build, f"ray{N}_default", N, 1, 1, DEFAULT_CRIT, 0, 400 + N % 97))
        add(f"ray{N}_rot", functools.partial(build, f"ray{N}_rot", N, 1, 1, _ROT[1] + (L1,), 0, 500 + N % 97))
    for name, fn in TIES.items():
        add(name, fn)
    return reg


# ------------------------------------------------------------------------------------------------ ties, degenerate inputs
def _tie_l1():
    """pd == gd on half of the rays: the L1 gradient there is 0 (torch's sign), +-a_d / N beside them."""
    N, a_d = 16, 4.0
    gt = np.zeros((N, 3))
    gt[:, 0], gt[:, 2] = 1.0, 3.0
    gt[13, 0] = 0.0
    d = np.array([0, 1, -1, 0, 2, 0, -3, 0, 0, 5, 0, -1, 0, 7, 0, 1]) / 256.0
    c = Case("tie_l1", 1, 1, DEFAULT_CRIT, 0, 1.0, 0.25, dict(FIXED_ALPHAS, a_d=a_d), gt[:, 2] + d, np.zeros((N, 2)), gt, 2.0 ** -8)
    c.closed["g_depth"] = (np.arange(N), a_d * np.sign(d) * gt[:, 0] / N)
    return c


def _tie_huber():
    """HUBER in all three slots with differences at +-delta, one float above and one below: the gradient is the difference
    clamped to [-delta, delta], so the three neighbours of +delta give d-, delta, delta."""
    delta = 0.25
    up, dn = float(np.nextafter(F(delta), F(1))), float(np.nextafter(F(delta), F(0)))
    d = np.array([0.0, delta, -delta, up, -up, dn, -dn, 2 * delta, -2 * delta, delta / 2, -delta / 2, 0.0, 0.0, 0.0, 0.0, 0.0])
    N = d.size
    gt = np.zeros((N, 3))
    gt[:11, 0] = 1.0                   # rays 0..10: depth and intensity ties (targets 0); rays 11..15 (gr = 0): ray-drop ties
    image = np.zeros((N, 2))
    image[:11, 1] = d[:11]
    image[11:, 0] = [delta, -delta, up, -dn, 3 * delta]
    al = dict(FIXED_ALPHAS, a_d=4.0, a_r=2.0, a_i=8.0)
    c = Case("tie_huber", 1, 1, (HUBER, HUBER, HUBER, L1), 0, 1.0, delta, al, d, image, gt, None)
    clip = lambda x: np.clip(x, -delta, delta)
    c.closed["g_depth"] = (np.arange(N), al["a_d"] * clip(d) * gt[:, 0] / N)
    gi = np.stack([al["a_r"] * clip(image[:, 0] - gt[:, 0]) / N, al["a_i"] * clip(image[:, 1]) * gt[:, 0] / N], axis=1)
    c.closed["g_image"] = (np.arange(N), gi)
    return c


def mask_boundary_floats():
    f = F(0.01)
    return float(f), float(np.nextafter(f, F(0)))


def _tie_mask():
    """Four 2 x 2 patches whose truth rows are (t, 0), t = +f, -f, +f-, -f- with f = fl(0.01f) and f- the float below it, scale 1
    (so gt grad x = t exactly).  |t| = f: mask off, gradient 0.  |t| = f-: mask on, and with prediction rows (2t, 0) for t > 0,
    (|t|, 0) for t < 0 the L1 residual u - w is |t| > 0: d loss / d depth = +-a_g / 8 on the two pixels of each row."""
    f, fm = mask_boundary_floats()
    a_g, N = 16.0, 16
    gt, depth = np.zeros((N, 3)), np.zeros(N)
    gt[:, 0] = 1.0
    want = np.zeros(N)
    for p, t in enumerate((f, -f, fm, -fm)):
        for row in range(2):
            n = p * 4 + row * 2
            gt[n, 2] = t
            depth[n] = 2 * t if t > 0 else -t
            if abs(t) < f:
                want[n], want[n + 1] = a_g / 8, -a_g / 8
    al = dict(FIXED_ALPHAS, a_g=a_g)
    image = np.stack([gt[:, 0], np.zeros(N)], axis=1)
    c = Case("tie_mask", 2, 2, DEFAULT_CRIT, GRAD, 1.0, 0.25, al, depth, image, gt, None, f32_threshold=True)
    per_ray = al["a_d"] * np.sign(depth - gt[:, 2]) / N
    c.closed["g_depth"] = (np.arange(N), want + per_ray)
    c.closed["g_image"] = (np.arange(N), np.zeros((N, 2)))
    return c


def _slope_patch(P, sobel, pred_value, dropped=()):
    """3 x 3 patches whose truth rows are (0, 1, 2) / 1024 m (mask fully on, Sobel or not) under a flat prediction."""
    N, scale = 9 * P, 0.5
    gt = np.zeros((N, 3))
    gt[:, 0] = 1.0
    gt[:, 2] = np.tile(np.array([0.0, 1.0, 2.0]) / 1024.0, 3 * P) * scale
    for p in dropped:
        gt[9 * p:9 * p + 9, 0] = 0.0
    depth = np.full(N, pred_value * scale)
    image = np.stack([gt[:, 0], np.zeros(N)], axis=1)
    al = dict(FIXED_ALPHAS, a_g=1.0)
    return Case("", 3, 3, DEFAULT_CRIT[:3] + (COS,), GRAD | (SOBEL if sobel else 0), scale, 2.0 ** -9, al, depth, image, gt,
                2.0 ** -12)


def _tie_cos_dropped(sobel):
    """COS with an all-dropped patch (of 4): it adds a_g / P to the loss and its gradient is exactly 0, not NaN."""
    c = _slope_patch(4, sobel, 0.0, dropped=(2,))
    rng = np.random.RandomState(7)
    c.depth = c.depth + rng.randint(0, 4, c.N) / 4096.0 * c.scale
    c.name = "tie_cos_dropped_" + ("sobel" if sobel else "plain")
    c.closed["g_depth"] = (np.arange(18, 27), np.zeros(9))
    return c


def _tie_cos_flat(sobel, P):
    """COS, flat prediction over sloped in-mask truth.  Without Sobel the prediction gradient |s| is 0 and d|s|/ds = 0 there:
    the structural term's gradient is exactly 0 (what remains is the per-ray L1 term, a_d sign(pd - gd) / N).  With Sobel
    and prediction 0, u = 0 and w != 0: the gradient is -a_g / P * w / (1e-8 |w|) through the stencil, near 1e8 and finite."""
    c = _slope_patch(P, sobel, 0.0 if sobel else 0.25)
    c.name = f"tie_cos_flat_{'sobel' if sobel else 'plain'}_{P}"
    if not sobel:
        pd, gd = c.depth * c.gt[:, 0], c.gt[:, 2] * c.gt[:, 0]
        per_ray = (F(c.alphas["a_d"]) * (np.sign(pd - gd) * c.gt[:, 0]).astype(F)) * (F(1) / F(c.N))   # one rounded product
        c.closed["g_depth"] = (np.arange(c.N), per_ray.astype(np.float64))
    return c


def _tie_cos_tiny_u():
    """COS with 0 < |u| < 1e-8: prediction rows (0, 1, 2) * 2^-30 m over the in-mask slope.  The value divides by the clamped
    norm, the second term of d cos / du by the clamped norm times the UNCLAMPED one."""
    c = _slope_patch(4, False, 0.0)
    c.depth = np.tile(np.array([0.0, 1.0, 2.0]) * 2.0 ** -30, 12) * c.scale
    c.name, c.lattice = "tie_cos_tiny_u", None
    return c


BCE_LOGITS = (0.0, 30.0, -30.0, 100.0, -100.0, 1000.0, -1000.0)


def _tie_bce_rays():
    """BCE in the three per-ray slots with logits 0, +-30, +-100, +-1000 against both targets — except (-100, 0): there the
    derivative sigmoid(-100) = 3.7e-44 is a float32 DENORMAL (5 bits), which no bound relative to the value can hold; its
    partner (-100, 1) keeps expf(100) in play.  expf overflows at +-1000: value and gradient must stay finite.
    Rays 0..15 carry the pairs in the ray-drop slot (target gr), rays 16..31 (gr = 1) in the depth and intensity slots."""
    pairs = [(x, y) for x in BCE_LOGITS for y in (0.0, 1.0) if (x, y) != (-100.0, 0.0)]
    H = 16
    assert len(pairs) <= H
    pairs += [(0.5, 1.0)] * (H - len(pairs))
    x, y = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    gt = np.zeros((2 * H, 3))
    gt[:H, 0], gt[H:, 0] = y, 1.0
    gt[H:, 2], gt[H:, 1] = y, y[::-1]
    image = np.zeros((2 * H, 2))
    image[:H, 0], image[H:, 0], image[H:, 1] = x, 0.5, x[::-1]
    depth = np.concatenate([np.zeros(H), x])
    al = dict(FIXED_ALPHAS, a_d=1.0, a_r=1.0, a_i=1.0)
    return Case("tie_bce_rays", 1, 1, (BCE, BCE, BCE, L1), 0, 1.0, 0.25, al, depth, image, gt, 2.0 ** -8)


def _tie_bce_grad():
    """BCE in the grad slot under Sobel: a prediction that depends on the column alone, with column profile c, has interior
    responses 4 (c[j+1] - c[j-1]) = 30, 100, 1000, 0, -1000, -100 and -30 at the right border (3 / 4 of that in the border
    rows), over an in-mask truth slope whose responses w are nonzero wherever the logit is negative."""
    px, py, P, scale = 3, 8, 3, 1.0
    prof = np.array([0.0, 0.0, 7.5, 25.0, 257.5, 25.0, 7.5, 0.0])
    N = px * py * P
    gt = np.zeros((N, 3))
    gt[:, 0] = 1.0
    gt[:, 2] = np.tile(np.arange(py) / 4096.0, px * P)
    depth = np.tile(prof, px * P)
    depth[2 * px * py:] *= 0.5            # third patch: half the logits
    image = np.stack([gt[:, 0], np.zeros(N)], axis=1)
    al = dict(FIXED_ALPHAS, a_d=2.0 ** -6, a_g=1.0)
    return Case("tie_bce_grad", px, py, DEFAULT_CRIT[:3] + (BCE,), SOBEL | GRAD, scale, 0.25, al, depth, image, gt, 2.0 ** -12)


def _named(fn, *a):
    return functools.partial(fn, *a)


TIES = {
    "tie_l1": _tie_l1, "tie_huber": _tie_huber, "tie_mask": _tie_mask,
    "tie_cos_dropped_plain": _named(_tie_cos_dropped, False), "tie_cos_dropped_sobel": _named(_tie_cos_dropped, True),
    "tie_cos_flat_plain_4": _named(_tie_cos_flat, False, 4), "tie_cos_flat_sobel_4": _named(_tie_cos_flat, True, 4),
    "tie_cos_flat_sobel_1": _named(_tie_cos_flat, True, 1),
    "tie_cos_tiny_u": _tie_cos_tiny_u, "tie_bce_rays": _tie_bce_rays, "tie_bce_grad": _tie_bce_grad,
}
_REG = _registry()


def all_names():
    return list(_REG)


@functools.lru_cache(maxsize=None)
def get_case(name):
    c = _REG[name]()
    c.name = name
    return c


def workspace_bytes(N):
    """lnh_lidar_loss_ex_workspace_bytes: one float per workgroup of 256 rays, in units of 16 bytes."""
    return (-(-N // WG) + 3) // 4 * 16
