"""Problems and references of tests/test_ragged_exact_gpu.py (NumPy only; conditions, coverage and sensitivity are asserted
without a GPU by tests/test_ragged_exact_cpu.py): the compositing kernels of the occupancy-grid path —
lnh_lidar_composite_rays_train_forward / _backward (one wave per ray, csrc/raymarch.hip), lnh_lidar_composite_rays and
lnh_alive_compact (the alive-ray evaluation, csrc/lidar_infer.hip) and the reference-shaped thread-per-ray compositors
lnh_composite_rays_train_forward / _backward and lnh_composite_rays (csrc/raymarch.hip).

TIER A — one right float32 value in any scan order.  expf is the only operation of these kernels IEEE does not pin, and the
only values every implementation agrees on are expf(-0) = 1 and expf(x) = 0 for very negative x.  So a sample is TRANSPARENT
(sigma = 0: alpha = 0) or OPAQUE (sigma = 2^20 with dt >= 2^-10: argument <= -1024, alpha = 1, and — the ragged walk has no
epsilon — T becomes exactly 0).  deltas[:, 0] and deltas[:, 1] are different powers of two, origins and directions multiples of
1/16 up to 2, positions multiples of 2^-8 below 4, features n / 16, upstream gradients small signed integers; weights_sum, depth
and image handed to the backward are dyadic values that are NOT the forward's.  Every sum then stays below 2^24 quanta of its
lattice (`RaggedCase.check_conditions`) and every partial sum in any scan or tree order is one float.

TIER B — general alpha: float64 restatements of the header's semantics (raymarching.cu:577-772 on the ragged samples) with a
bound PER ELEMENT from the standard rounding model (`walk_bounds`, `lidar_bounds`, `rgb_bounds`).
"""
import functools

import numpy as np

from render_exact_cases import EXPF_ULPS, TINY, U, gamma

F = np.float32
ROUND, WG_RAYS = 64, 4             # samples per round of a wave, rays per workgroup of the wave-per-ray kernels
OPAQUE = float(2 ** 20)
TAIL_ROWS = 3                      # rows M .. M + 2 of every sample buffer: owned by nobody (and read by nobody)
INF = float("inf")

COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
I0_SET = (0, 62, 63, 64, 65, 127, 128)          # and count - 1, and none
N_SET = (1, 3, 4, 5, 9)
K_SET = (1, 2, 3)
THRESHOLDS = (1e-4, 0.0, 1.0)
N_STEPS = (1, 2, 3, 8, 24, 64, 100, 130)
RGB_N = (1, 63, 64, 65)
COMPACT_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4096)
TIE = 2.0 ** -13                                  # the transmittance a ray is started at to sit ON the threshold
TIE_ABOVE = float(np.nextafter(F(TIE), F(1)))

# The classic mistakes of such kernels, each applied by name to the NumPy models below (tests/test_ragged_exact_cpu.py asserts
# that each changes an expected tier-A array; the same mistakes compiled into the library all fail the GPU file: DESIGN.md 8).
MISTAKES = ("Tc_dropped", "dc_dropped", "accc_dropped", "stop_excluded", "le_threshold", "no_break", "Ti_for_Tn",
            "capacity_ge", "table_row", "feat_stride1", "no_origin", "dt_col1", "rgb_depth_col0", "alive_trans_not_stored",
            "alive_no_gshift", "alive_short_rule", "compact_wave_order")


def width_of(n_step):
    """Lanes per ray of lnh_lidar_composite_rays: the power of two that holds a round's samples, a wave at most."""
    W = 1
    while W < n_step and W < 64:
        W *= 2
    return W


# ================================================================================================ tier A: the problems
def ray_specs():
    """(count, i0): every count with the first opaque sample at every position class that exists (None = no opaque sample)."""
    specs = []
    for c in COUNTS:
        for i0 in [None] + sorted({p for p in I0_SET + (c - 1,) if 0 <= p < c}):
            specs.append((c, i0))
    return specs


def i0_classes(count, i0):
    if i0 is None:
        return {"none"}
    k = {i0} & set(I0_SET)
    if i0 == count - 1:
        k.add("count-1")
    return k


def table_specs():
    """The ray tables: (N, [(count, i0, role)]).  Sizes walk through N_SET; a table of N >= 3 rays holds N - 2 rays of
    ray_specs() — the last of them ends at M exactly ('last') —, one ray that ends at M + 1 ('dropped') and one empty ray; a
    one-ray table holds a ray that ends at M; two more one-ray tables hold a dropped and an empty ray alone."""
    specs = ray_specs()
    tables, pos, t = [], 0, 0
    sizes = (9, 5, 4, 3, 1)
    while pos < len(specs):
        N = sizes[t % len(sizes)]
        need = N - 2 if N >= 3 else 1
        rays = [specs[(pos + j) % len(specs)] for j in range(need)]
        pos += need
        assert N >= 4 or rays[0][0] > 0, "the ray that ends at M has samples"
        rows = [(c, i0, "kept") for c, i0 in rays]
        k = max(range(len(rows)), key=lambda j: (rows[j][0] > 0, j))            # the last ray with samples ends at M
        rows[k] = rows[k][:2] + ("last",)
        if N >= 3:
            dc, di0 = specs[(11 * t + 5) % len(specs)]
            if dc == 0:
                dc, di0 = 65, 63
            rows += [(dc, di0, "dropped"), (0, None, "empty")]
        tables.append((N, rows))
        t += 1
    tables.append((1, [(65, 63, "dropped")]))
    tables.append((1, [(0, None, "empty")]))
    return tables


def _dyadic(rng, lo, hi, q, shape, nonzero=False):
    v = rng.integers(lo, hi + 1, shape)
    if nonzero:
        v = np.where(v == 0, hi, v)
    return v / float(q)


class RaggedCase:
    """One ray table over one set of sample buffers.  `rows`: (count, i0, role) per ray; the table lists the rays in an arrival
    order that is not the order of their indices, samples lie at `offset` with unowned rows between the rays and behind M."""

    def __init__(self, rows, K, seed):
        self.K, self.N = K, len(rows)
        for salt in range(64):
            rng = np.random.default_rng(1000003 * seed + 1009 * K + salt)
            self._build(rows, rng)
            if self._distinct():
                break
        else:
            raise AssertionError("no seed gives distinct gradient terms")
        self.salt = salt

    def _build(self, rows, rng):
        N, K = self.N, self.K
        index = rng.permutation(N)
        if N > 1 and np.array_equal(index, np.arange(N)):
            index = np.roll(index, 1)
        order = list(rng.permutation(N))                                          # memory order of the rays
        self.count = np.array([r[0] for r in rows])
        self.i0 = [r[1] for r in rows]
        self.role = [r[2] for r in rows]
        offset = np.zeros(N, np.int64)
        cur = 0
        tail = [j for j in order if self.role[j] == "last"]
        for j in [j for j in order if self.role[j] in ("kept", "empty")] + tail:
            cur += int(rng.integers(1, 4))                                        # unowned rows in front of every ray
            offset[j] = cur
            cur += int(self.count[j])
        M = cur if tail else cur + 2
        for j in range(N):
            if self.role[j] == "dropped":
                if self.count[j] > M:                                             # (its rows start at row 1)
                    self.count[j], self.i0[j] = M, None
                offset[j] = M + 1 - self.count[j]
        self.M, self.rows_total = M, M + TAIL_ROWS
        R = self.rows_total
        self.index, self.offset = index, offset
        table_order = rng.permutation(N)                                          # arrival order of the table rows
        if N > 1 and np.array_equal(index[table_order], np.arange(N)):
            table_order = np.roll(table_order, 1)
        self.rays = np.stack([index[table_order], offset[table_order], self.count[table_order]], 1).astype(np.int32)
        self.row_of = np.argsort(table_order)                                     # table row of ray j
        self.owner = np.full(R, -1)
        for j in range(N):
            if self.role[j] in ("kept", "last"):
                self.owner[offset[j]:offset[j] + self.count[j]] = j
        self.sigma = np.where(self.owner >= 0, 0.0, OPAQUE)                       # an unowned row is loud if it is read
        for j in range(N):
            if self.i0[j] is not None and self.role[j] != "dropped":
                self.sigma[offset[j] + self.i0[j]] = OPAQUE
                if (j % 2 or self.i0[j] % ROUND == ROUND - 1) and self.i0[j] + 1 < self.count[j]:
                    self.sigma[offset[j] + self.i0[j] + 1] = OPAQUE               # behind i0 T is 0: opaque or not, w = 0
        a = rng.integers(4, 11, R)
        b = 3 + (a - 3 + rng.integers(1, 8, R)) % 8
        self.deltas = np.stack([2.0 ** -a, 2.0 ** -b], 1)
        self.xyz = _dyadic(rng, -1023, 1023, 256, (R, 3))
        self.o = _dyadic(rng, -32, 32, 16, (N, 3))
        self.d = _dyadic(rng, -32, 32, 16, (N, 3), nonzero=True)
        self.feats = _dyadic(rng, 1, 15, 16, (R, K))
        sign = lambda shape: rng.choice([-1.0, 1.0], shape)
        self.g_ws, self.g_depth = sign(N) * rng.integers(1, 5, N), sign(N) * rng.integers(1, 5, N)
        self.g_image = sign((N, K)) * rng.integers(1, 5, (N, K))
        # what the backward is HANDED as the forward's results: dyadic, and not the forward's
        self.ws_final = np.full(N, 0.5)
        self.d_final = sign(N) * rng.integers(1, 65, N) / 16.0
        self.fin = sign((N, K)) * rng.integers(17, 33, (N, K)) / 16.0

    def finals(self):
        return self.ws_final, self.d_final, self.fin

    def z(self):
        """(xyz - o) . d of every owned row, exact; NaN elsewhere."""
        z = np.full(self.rows_total, np.nan)
        for j in range(self.N):
            s = slice(self.offset[j], self.offset[j] + self.count[j])
            if self.role[j] in ("kept", "last"):
                z[s] = ((self.xyz[s] - self.o[self.index[j]]) * self.d[self.index[j]]).sum(-1)
        return z

    def _distinct(self):
        """Every gradient element is non-zero (T_thresh = 0: the whole ray), and through i0 the gradient of a sample differs
        from its neighbour's and from the one a round away.  (Behind i0 it is dt_i times ONE non-zero number: T_{i+1} = 0 and
        the prefix stands still there.)"""
        g = lidar_reference(self, 0.0, np.float64, self.finals())["grad_sigmas"]
        for j in range(self.N):
            if self.role[j] in ("kept", "last"):
                v = g[self.offset[j]:self.offset[j] + self.count[j]]
                head = v if self.i0[j] is None else v[:self.i0[j] + 1]
                if np.any(v == 0) or np.any(head[1:] == head[:-1]) or np.any(head[ROUND:] == head[:-ROUND]):
                    return False
        return True

    def check_conditions(self):
        """The conditions under which the closed forms are the ONE float32 answer."""
        R, N, K = self.rows_total, self.N, self.K
        assert set(np.unique(self.sigma)) <= {0.0, OPAQUE}
        lg = np.log2(self.deltas)
        assert np.array_equal(lg, np.rint(lg)) and lg.min() >= -10 and lg.max() <= -3, "deltas are powers of two >= 2^-10"
        assert np.all(self.deltas[:, 0] != self.deltas[:, 1]), "the two delta columns differ on every sample"
        arg = self.sigma[:, None] * self.deltas
        assert np.all((arg == 0) | (arg >= 1024.0)), "expf argument is -0 or <= -1024, whichever column is read"
        for v, q, top in ((self.o, 16, 2), (self.d, 16, 2), (self.xyz, 256, 4), (self.feats, 16, 1)):
            assert np.array_equal(v * q, np.rint(v * q)) and np.abs(v).max() <= top
        assert np.abs(self.xyz).max() < 4 and self.feats.min() > 0
        for g in (self.g_ws, self.g_depth, self.g_image):
            assert np.array_equal(g, np.rint(g)) and np.abs(g).min() >= 1 and np.abs(g).max() <= 4
        assert np.all(self.ws_final == 0.5)
        assert np.array_equal(self.d_final * 16, np.rint(self.d_final * 16)) and np.array_equal(self.fin * 16, np.rint(self.fin * 16))
        # z: three products on the lattice 2^-12, |xyz - o| < 6, |d| <= 2
        zq = 2.0 ** -12
        for j in range(N):
            if self.role[j] not in ("kept", "last"):
                continue
            i, s = self.index[j], slice(self.offset[j], self.offset[j] + self.count[j])
            t = (self.xyz[s] - self.o[i]) * self.d[i]
            assert np.array_equal(t / zq, np.rint(t / zq)) and np.all(np.abs(t).sum(-1) / zq < 2.0 ** 24)
            z = t.sum(-1)
            # the forward sums: at most one weight is 1, the rest 0 — and the running column-1 depth of the RGB kernels
            assert np.all(np.abs(z) / zq < 2.0 ** 24) and self.deltas[s, 1].sum() / 2.0 ** -10 < 2.0 ** 24
            # the gradient of sample i: sum |addends| with T_{i+1} <= 1 and the prefixes at most |z_i0|, |f_i0|
            zmax, fmax = np.abs(z).max(initial=0.0), self.feats[s].max(initial=0.0)
            A = (np.abs(self.g_ws[i]) * 0.5 + np.abs(self.g_depth[i]) * (2 * zmax + np.abs(self.d_final[i]))
                 + (np.abs(self.g_image[i]) * (2 * fmax + np.abs(self.fin[i]))).sum())
            assert A / zq < 2.0 ** 24, "sum |addends| of a gradient element stays below 2^24 quanta"
        assert self.owner[self.M:].max(initial=-1) == -1
        if N >= 3:
            assert {"last", "dropped", "empty"} <= set(self.role), "every table of three rays or more carries all three"
        for j in range(N):
            if self.role[j] == "last":
                assert self.offset[j] + self.count[j] == self.M
            if self.role[j] == "dropped":
                assert self.offset[j] + self.count[j] == self.M + 1 and self.offset[j] >= 0
        if N > 1:
            assert not np.array_equal(self.rays[:, 0], np.arange(N)), "arrival order differs from ray index"
        assert np.array_equal(np.sort(self.rays[:, 0]), np.arange(N))
        gaps = np.flatnonzero(self.owner[:self.M] < 0)
        assert len(gaps) >= 1 and TAIL_ROWS >= 1, "unowned rows between rays and behind the last ray"


def _kept(rays_row, M, mistake=None):
    index, offset, count = (int(v) for v in rays_row)
    over = offset + count >= M if mistake == "capacity_ge" else offset + count > M
    return count != 0 and not over


# ================================================================================================ the semantics, restated
def _thr(T_thresh, dtype):
    """The threshold the kernels compare with is a float32 argument."""
    return dtype(F(T_thresh))


def lidar_reference(c, T_thresh, dtype=np.float64, finals=None):
    """lnh_lidar_composite_rays_train_forward / _backward as the header states them (raymarching.cu:577-772 semantics on the
    marcher's samples, K channels, absolute depth), one serial walk per ray:
        alpha_i = 1 - exp(-sigma_i dt_i),  T_0 = 1,  T_{i+1} = T_i (1 - alpha_i),  w_i = alpha_i T_i,
        the sample that takes T below T_thresh is the last one that counts (strict <),
        g_i = dt_i (g_ws (1 - ws_final) + g_d (T_{i+1} z_i - (d_final - D_i)) + sum_k g_k (T_{i+1} f_ik - (fin_k - A_ik))),
    D_i, A_ik the sums through sample i.  A ray with count = 0 or offset + count > M has zero outputs and writes no gradient.
    NaN in the gradients = never written.  `finals` = (weights_sum, depth, image) handed to the backward (default: the
    forward's own).  Run in float32 on a tier-A problem this IS the expected output: every operation is exact there."""
    N, K, R = c.N, c.K, c.rows_total
    sig, dl, xyz, feats = (np.asarray(a, dtype) for a in (c.sigma, c.deltas, c.xyz, c.feats))
    o, d = np.asarray(c.o, dtype), np.asarray(c.d, dtype)
    ws, dep, img = np.zeros(N, dtype), np.zeros(N, dtype), np.zeros((N, K), dtype)
    walks = {}
    thr = _thr(T_thresh, dtype)
    for row in c.rays:
        index, offset, count = (int(v) for v in row)
        if not _kept(row, c.M):
            continue
        s = slice(offset, offset + count)
        with np.errstate(under="ignore"):
            alpha = dtype(1) - np.exp(-sig[s] * dl[s, 0])
        om = dtype(1) - alpha
        Tn = np.cumprod(om, dtype=dtype)
        T = np.concatenate([[dtype(1)], Tn[:-1]])
        below = np.flatnonzero(Tn < thr)
        last = int(below[0]) if len(below) else count - 1
        keep = np.arange(count) <= last
        w = np.where(keep, alpha * T, dtype(0))
        t = (xyz[s] - o[index]) * d[index]
        z = (t[:, 0] + t[:, 1]) + t[:, 2]
        ws[index], dep[index], img[index] = w.sum(), (w * z).sum(), (w[:, None] * feats[s]).sum(0)
        walks[index] = dict(s=s, alpha=alpha, om=om, T=T, Tn=Tn, keep=keep, w=w, z=z, t=t, last=last)
    out = {"weights_sum": ws, "depth": dep, "image": img, "walks": walks}
    wsf, dfin, fin = (np.asarray(a, dtype) for a in (finals if finals is not None else (ws, dep, img)))
    gs, gf = np.full(R, np.nan, dtype), np.full((R, K), np.nan, dtype)
    g_ws, g_d, g_im = (np.asarray(a, dtype) for a in (c.g_ws, c.g_depth, c.g_image))
    for index, k in walks.items():
        s, w, keep = k["s"], k["w"], k["keep"]
        D = np.cumsum(w * k["z"], dtype=dtype)
        A = np.cumsum(w[:, None] * feats[s], axis=0, dtype=dtype)
        g = g_ws[index] * (dtype(1) - wsf[index]) + g_d[index] * (k["Tn"] * k["z"] - (dfin[index] - D))
        for ch in range(K):
            g = g + g_im[index, ch] * (k["Tn"] * feats[s][:, ch] - (fin[index, ch] - A[:, ch]))
        gs[s] = np.where(keep, dl[s, 0] * g, np.nan)
        gf[s] = np.where(keep[:, None], g_im[index][None, :] * w[:, None], np.nan)
        k["D"], k["A"] = D, A
    out["grad_sigmas"], out["grad_feats"] = gs, gf
    return out


def lidar_closed_forms(c, T_thresh):
    """The tier-A answers written down directly: i0 = the first opaque sample of a kept ray.  weights_sum = 1, depth = z_i0,
    image = f_i0 (all 0 without one).  Gradient of sample i, with T_{i+1} and the prefix by position — in front of i0: 1 and 0;
    at i0: 0 and z_i0; behind it: 0 and z_i0 —; written through i0 (T_thresh in (0, 1]), through the whole ray (T_thresh = 0),
    and an all-transparent ray is written whole whatever the threshold (T stays 1, the comparison is strict)."""
    N, K, R = c.N, c.K, c.rows_total
    ws, dep, img = np.zeros(N), np.zeros(N), np.zeros((N, K))
    gs, gf = np.full(R, np.nan), np.full((R, K), np.nan)
    z = c.z()
    for j in range(N):
        if c.role[j] not in ("kept", "last") or c.count[j] == 0:
            continue
        i, off, cnt, i0 = c.index[j], c.offset[j], c.count[j], c.i0[j]
        n_written = cnt if (i0 is None or F(T_thresh) <= 0) else i0 + 1
        for p in range(n_written):
            r = off + p
            front = i0 is None or p < i0
            Tn, Dz, Af = (1.0, 0.0, np.zeros(K)) if front else (0.0, z[off + i0], c.feats[off + i0])
            g = c.g_ws[i] * 0.5 + c.g_depth[i] * (Tn * z[r] - (c.d_final[i] - Dz))
            g += (c.g_image[i] * (Tn * c.feats[r] - (c.fin[i] - Af))).sum()
            gs[r] = c.deltas[r, 0] * g
            gf[r] = c.g_image[i] * (1.0 if p == i0 else 0.0)
        if i0 is not None:
            ws[i], dep[i], img[i] = 1.0, z[off + i0], c.feats[off + i0]
    return {"weights_sum": ws, "depth": dep, "image": img, "grad_sigmas": gs, "grad_feats": gf}


def simulate(c, T_thresh, mistake=None, dtype=F, finals=None, drop=None):
    """A model of the STRUCTURE of k_lidar_composite_ragged_fwd / _bwd: rounds of 64 samples, the carries Tc, dc and accc
    between them, the stop ballot, the table walk.  `mistake` names one of MISTAKES; `drop` = (carry, round) resets one carry
    in front of one round (the teeth of the tier-B bounds).  Sums are taken in sample order."""
    N, K, R, M = c.N, c.K, c.rows_total, c.M
    sig, dl, xyz = (np.asarray(a, dtype) for a in (c.sigma, c.deltas, c.xyz))
    feats = np.asarray(c.feats, dtype)
    flat = np.concatenate([feats.reshape(-1), np.zeros(K, dtype)])
    o, d = np.asarray(c.o, dtype), np.asarray(c.d, dtype)
    g_ws, g_d, g_im = (np.asarray(a, dtype) for a in (c.g_ws, c.g_depth, c.g_image))
    if finals is None:
        finals = lidar_reference(c, T_thresh, dtype)
        finals = (finals["weights_sum"], finals["depth"], finals["image"])
    wsf, dfin, fin = (np.asarray(a, dtype) for a in finals)
    ws, dep, img = np.full(N, np.nan, dtype), np.full(N, np.nan, dtype), np.full((N, K), np.nan, dtype)
    gs, gf = np.full(R, np.nan, dtype), np.full((R, K), np.nan, dtype)
    thr = _thr(T_thresh, dtype)
    one, zero = dtype(1), dtype(0)
    for n, row in enumerate(c.rays):
        index, offset, count = (int(v) for v in row)
        if mistake == "table_row":
            index = n
        a_ws, a_d, a_img = zero, zero, np.zeros(K, dtype)
        if _kept(row, M, mistake):
            oo = np.zeros(3, dtype) if mistake == "no_origin" else o[index]
            Tc, dc, accc = one, zero, np.zeros(K, dtype)
            for rd, base in enumerate(range(0, count, ROUND)):
                if drop is not None and drop[1] == rd:
                    if drop[0] == "Tc":
                        Tc = one
                    elif drop[0] == "dc":
                        dc = zero
                    else:
                        accc = np.zeros(K, dtype)
                m = min(ROUND, count - base)
                s = slice(offset + base, offset + base + m)
                dt = dl[s, 1 if mistake == "dt_col1" else 0]
                with np.errstate(under="ignore"):
                    alpha = one - np.exp(-sig[s] * dt)
                rows_i = np.arange(offset + base, offset + base + m)
                if mistake == "feat_stride1":
                    f = np.stack([flat[rows_i + k] for k in range(K)], 1)
                else:
                    f = feats[s]
                t = (xyz[s] - oo) * d[index]
                z = (t[:, 0] + t[:, 1]) + t[:, 2]
                incl = np.cumprod(one - alpha, dtype=dtype)
                Tn, T = Tc * incl, Tc * np.concatenate([[one], incl[:-1]])
                stop = np.flatnonzero(Tn <= thr if mistake == "le_threshold" else Tn < thr)
                last = int(stop[0]) if len(stop) else ROUND - 1
                use = np.arange(m) < last if mistake == "stop_excluded" else np.arange(m) <= last
                w = np.where(use, alpha * T, zero)
                a_ws, a_d, a_img = a_ws + w.sum(), a_d + (w * z).sum(), a_img + (w[:, None] * f).sum(0)
                D = dc + np.cumsum(w * z, dtype=dtype)
                A = accc + np.cumsum(w[:, None] * f, axis=0, dtype=dtype)
                Tg = T if mistake == "Ti_for_Tn" else Tn
                g = g_ws[index] * (one - wsf[index]) + g_d[index] * (Tg * z - (dfin[index] - D))
                for ch in range(K):
                    g = g + g_im[index, ch] * (Tg * f[:, ch] - (fin[index, ch] - A[:, ch]))
                gs[s] = np.where(use, dt * g, gs[s])
                gf[s] = np.where(use[:, None], g_im[index][None, :] * w[:, None], gf[s])
                if len(stop) and mistake != "no_break":
                    break
                if mistake != "dc_dropped":
                    dc = D[-1]
                if mistake != "accc_dropped":
                    accc = A[-1]
                if mistake != "Tc_dropped":
                    Tc = Tn[-1]
        ws[index], dep[index], img[index] = a_ws, a_d, a_img
    return {"weights_sum": ws, "depth": dep, "image": img, "grad_sigmas": gs, "grad_feats": gf}


# ---- the reference-shaped RGB compositors: serial loops, three channels, relative depth, no depth gradient
def rgb_reference(c, T_thresh, dtype=np.float64, finals=None, mistake=None):
    """lnh_composite_rays_train_forward / _backward (raymarching.cu:577-772): per ray, in sample order,
        alpha = 1 - exp(-sigma dl0),  w = alpha T,  t += dl1,  depth += w t,  T *= 1 - alpha,  stop once T < T_thresh;
        g_i = dl0 (sum_k g_k (T_{i+1} c_ik - (fin_k - acc_ik)) + g_ws (1 - ws_final)), written through the stop sample."""
    assert c.K == 3
    N, R = c.N, c.rows_total
    sig, dl, rgb = (np.asarray(a, dtype) for a in (c.sigma, c.deltas, c.feats))
    ws, dep, img = np.zeros(N, dtype), np.zeros(N, dtype), np.zeros((N, 3), dtype)
    gs, gc = np.full(R, np.nan, dtype), np.full((R, 3), np.nan, dtype)
    thr = _thr(T_thresh, dtype)
    walks = {}
    for row in c.rays:
        index, offset, count = (int(v) for v in row)
        if not _kept(row, c.M):
            continue
        s = slice(offset, offset + count)
        with np.errstate(under="ignore"):
            alpha = dtype(1) - np.exp(-sig[s] * dl[s, 0])
        Tn = np.cumprod(dtype(1) - alpha, dtype=dtype)
        T = np.concatenate([[dtype(1)], Tn[:-1]])
        below = np.flatnonzero(Tn < thr)
        last = int(below[0]) if len(below) else count - 1
        keep = np.arange(count) <= last
        w = np.where(keep, alpha * T, dtype(0))
        t = np.cumsum(dl[s, 0 if mistake == "rgb_depth_col0" else 1], dtype=dtype)
        ws[index] = np.cumsum(w, dtype=dtype)[-1]
        dep[index] = np.cumsum(w * t, dtype=dtype)[-1]
        img[index] = np.cumsum(w[:, None] * rgb[s], axis=0, dtype=dtype)[-1]
        walks[index] = dict(s=s, alpha=alpha, T=T, Tn=Tn, keep=keep, w=w, t=t)
    wsf, _, fin = (np.asarray(a, dtype) for a in (finals if finals is not None else (ws, dep, img)))
    g_ws, g_im = np.asarray(c.g_ws, dtype), np.asarray(c.g_image, dtype)
    for index, k in walks.items():
        s, w, keep = k["s"], k["w"], k["keep"]
        A = np.cumsum(w[:, None] * rgb[s], axis=0, dtype=dtype)
        g = g_im[index, 0] * (k["Tn"] * rgb[s][:, 0] - (fin[index, 0] - A[:, 0]))
        for ch in (1, 2):
            g = g + g_im[index, ch] * (k["Tn"] * rgb[s][:, ch] - (fin[index, ch] - A[:, ch]))
        g = g + g_ws[index] * (dtype(1) - wsf[index])
        gs[s] = np.where(keep, dl[s, 0] * g, np.nan)
        gc[s] = np.where(keep[:, None], g_im[index][None, :] * w[:, None], np.nan)
        k["A"] = A
    return {"weights_sum": ws, "depth": dep, "image": img, "grad_sigmas": gs, "grad_rgbs": gc, "walks": walks}


# ================================================================================================ cases
@functools.lru_cache(maxsize=None)
def get_case(tid, K):
    N, rows = table_specs()[tid]
    c = RaggedCase(rows, K, seed=tid)
    assert c.N == N
    c.check_conditions()
    return c


def table_ids():
    return list(range(len(table_specs())))


@functools.lru_cache(maxsize=None)
def get_rgb_case(N):
    """N rays (N around the 64 threads of a workgroup) that walk through ray_specs(), with a dropped, an empty and a last ray."""
    specs = ray_specs()
    if N == 1:
        rows = [(129, 64, "last")]
    else:
        rows = [specs[(3 * j + N) % len(specs)] + ("kept",) for j in range(N - 2)]
        k = max(range(len(rows)), key=lambda j: (rows[j][0] > 0, j))
        rows[k] = rows[k][:2] + ("last",)
        rows += [(65, 63, "dropped"), (0, None, "empty")]
    c = RaggedCase(rows, 3, seed=500 + N)
    c.check_conditions()
    return c


def coverage():
    """What the tier-A tables meet (kept rays only)."""
    met = {"count": set(), "i0": set(), "pair": set(), "N": set(), "roles": {}, "K": set(K_SET)}
    for tid in table_ids():
        c = get_case(tid, 1)
        met["N"].add(c.N)
        met["roles"][tid] = set(c.role)
        for j in range(c.N):
            if c.role[j] in ("kept", "last", "empty"):
                met["count"].add(int(c.count[j]))
                met["i0"] |= i0_classes(c.count[j], c.i0[j])
                met["pair"].add((int(c.count[j]), c.i0[j]))
    return met


# ================================================================================================ the alive-ray evaluation
def alive_model(p, dtype=F, mistake=None):
    """lnh_lidar_composite_rays on one call `p` (a dict: n_alive_max, n_step, N, K, T_thresh, alive_count, rays_alive, rays_t,
    rays, sigmas, feats, deltas, xyzs, o, d and the state weights_sum, depth, image, trans): the state and the alive list after
    it.  Slot n < min(max(alive_count, 0), n_alive_max) is a ray if rays[n, 0] is a ray id and equals rays_alive[n]; a ray's
    samples are composited from the carried transmittance in groups of W lanes; it is dead when it stopped, when count < n_step or
    when rays_t holds +inf; a slot that is no ray is marked dead and its state is not touched."""
    n_step, N, K = p["n_step"], p["N"], p["K"]
    W = width_of(n_step)
    n_alive = min(max(int(p["alive_count"]), 0), p["n_alive_max"])
    sig, dl, xyz, feats = (np.asarray(p[k], dtype) for k in ("sigmas", "deltas", "xyzs", "feats"))
    o, d = np.asarray(p["o"], dtype), np.asarray(p["d"], dtype)
    ws, dep, img, trans = (np.array(p[k], dtype) for k in ("weights_sum", "depth", "image", "trans"))
    alive = np.array(p["rays_alive"], np.int32)
    thr = _thr(p["T_thresh"], dtype)
    one, zero = dtype(1), dtype(0)
    per_wave = 64 // W
    st = {}
    for n in range(n_alive):
        index, offset, count = (int(v) for v in p["rays"][n])
        ray = 0 <= index < N and int(alive[n]) == index
        if not ray or offset + count > p["n_alive_max"] * n_step:
            count = 0
        st[n] = dict(index=index, offset=offset, count=count, ray=ray, Tc=trans[index] if ray else one, stopped=False,
                     a_ws=zero, a_d=zero, a_img=np.zeros(K, dtype))
    for base in range(0, n_step, W):
        masks = {}
        for n in range(n_alive):
            k = st[n]
            m = 0 if k["stopped"] else max(min(W, k["count"] - base), 0)
            s = slice(k["offset"] + base, k["offset"] + base + m)
            with np.errstate(under="ignore"):
                alpha = one - np.exp(-sig[s] * dl[s, 0])
            incl = np.cumprod(one - alpha, dtype=dtype)
            Tn, T = k["Tc"] * incl, k["Tc"] * np.concatenate([[one], incl[:-1]])[:m]
            masks[n] = (m, s, alpha, Tn, T, Tn < thr)
        for n in range(n_alive):
            k = st[n]
            m, s, alpha, Tn, T, below = masks[n]
            if mistake == "alive_no_gshift":                     # every group reads the ballot bits of the wave's first group
                first = n - n % per_wave
                b0 = masks[first][5]
                below = np.array([j < len(b0) and bool(b0[j]) for j in range(m)], bool)
                stop_any = bool(b0.any())
                last = int(np.flatnonzero(b0)[0]) if stop_any else W - 1
            else:
                stop_any = bool(below.any())
                last = int(np.flatnonzero(below)[0]) if stop_any else W - 1
            if m:
                t = (xyz[s] - o[k["index"]]) * d[k["index"]]
                z = (t[:, 0] + t[:, 1]) + t[:, 2]
                w = np.where(np.arange(m) <= last, alpha * T, zero)
                k["a_ws"], k["a_d"] = k["a_ws"] + w.sum(), k["a_d"] + (w * z).sum()
                k["a_img"] = k["a_img"] + (w[:, None] * feats[s]).sum(0)
            Tnext = k["Tc"] if m == 0 else Tn[min(last, m - 1)]
            if not k["stopped"]:
                k["Tc"] = Tnext
            if stop_any:
                k["stopped"] = True
    for n in range(n_alive):
        k = st[n]
        if not k["ray"]:
            alive[n] = -1
            continue
        i = k["index"]
        if k["count"]:
            ws[i], dep[i], img[i] = ws[i] + k["a_ws"], dep[i] + k["a_d"], img[i] + k["a_img"]
            if not (mistake == "alive_trans_not_stored" and k["stopped"]):
                trans[i] = k["Tc"]
        dead = k["stopped"] or (k["count"] < n_step and mistake != "alive_short_rule") or not (p["rays_t"][i] < INF)
        if dead:
            alive[n] = -1
    return {"weights_sum": ws, "depth": dep, "image": img, "trans": trans, "rays_alive": alive}


def alive_rounds(c, n_step, T_thresh=1e-4, dtype=F, mistake=None):
    """The kept and empty rays of a table, cut into rounds of n_step samples: one call per round, the `rays` table, the sample
    buffers and rays_t rebuilt per round as k_lidar_march_rays writes them (slot n owns rows [n n_step, (n + 1) n_step), rows a
    slot does not fill carry delta = 0, (0, 0, 0) beyond the alive count, rays_t = +inf where the walk ended).  A ray whose
    samples end with a full round gets the mark at once if its index is odd (the max_steps rule) and an empty round otherwise.
    Yields (call, expected state after it); the survivors are compacted in NumPy."""
    N, K = c.N, c.K
    ids = [int(c.index[j]) for j in range(N) if c.role[j] in ("kept", "last", "empty")]
    ids.sort(key=lambda i: (i * 7) % 11)                                       # slot order is not ray order
    by_index = {int(c.index[j]): j for j in range(N)}
    n_max = len(ids)
    state = {"weights_sum": np.zeros(N, dtype), "depth": np.zeros(N, dtype), "image": np.zeros((N, K), dtype),
             "trans": np.ones(N, dtype)}
    done = {i: 0 for i in ids}
    alive = list(ids)
    R = n_max * n_step
    rng = np.random.default_rng(77 + n_step)
    for _ in range(1000):
        if not alive:
            return
        rays = np.zeros((N, 3), np.int32)
        sig = np.full(R, OPAQUE)
        dl = np.zeros((R, 2))
        xyz = _dyadic(rng, -1023, 1023, 256, (R, 3))
        feats = _dyadic(rng, 1, 15, 16, (R, K))
        rays_t = np.full(N, 0.5)
        for n, i in enumerate(alive):
            j = by_index[i]
            m = min(n_step, int(c.count[j]) - done[i])
            src = slice(c.offset[j] + done[i], c.offset[j] + done[i] + m)
            dst = slice(n * n_step, n * n_step + m)
            sig[dst], dl[dst], xyz[dst], feats[dst] = c.sigma[src], c.deltas[src], c.xyz[src], c.feats[src]
            rays[n] = (i, n * n_step, m)
            done[i] += m
            if m < n_step or (done[i] == c.count[j] and i % 2):
                rays_t[i] = INF
        stale = np.full(n_max, 7, np.int32)                                       # what lies behind the alive count stays
        stale[:len(alive)] = alive
        p = dict(n_alive_max=n_max, n_step=n_step, N=N, K=K, T_thresh=T_thresh, alive_count=len(alive), rays_alive=stale,
                 rays_t=rays_t, rays=rays, sigmas=sig, feats=feats, deltas=dl, xyzs=xyz, o=c.o, d=c.d, **state)
        e = alive_model(p, dtype, mistake)
        yield p, e
        state = {k: e[k] for k in ("weights_sum", "depth", "image", "trans")}
        alive = [int(v) for v in e["rays_alive"][:len(alive)] if v >= 0]
    raise AssertionError("the alive loop does not end")


def alive_final(c, n_step, T_thresh=1e-4, dtype=F, mistake=None):
    e = None
    calls = 0
    for _, e in alive_rounds(c, n_step, T_thresh, dtype, mistake):
        calls += 1
    return e, calls


ALIVE_STATE_THRESHOLDS = (TIE, TIE_ABOVE)
ALIVE_STATE_COUNTS = ("all", "clipped", "zero", "negative", "fewer")


def alive_state_case(T_thresh, count_kind, K=2):
    """One call with n_step = 8 (W = 8: eight groups a wave) on caller-made state.  Slots 0 .. 15: eight rays that stop at lanes
    0 .. 7 of their own group, each next to a transparent ray that does not; then rays started at trans 1/2 and 2^-13 with
    non-zero running sums, opaque and transparent (the transparent one at 2^-13 sits ON T_thresh = 2^-13 and must go on; the
    float above stops it at its first sample, which stores trans); a short ray, an empty ray, a ray with the +inf mark after a
    full round, a stale slot.  `count_kind`: alive_count = the slots, more than n_alive_max, 0, negative, fewer."""
    n_step = 8
    rng = np.random.default_rng(4242)
    slots = []                                    # (kind, i0, trans, count, rays_t)
    for j in range(8):
        slots += [("stop", j, 1.0, 8, 0.5), ("through", None, 1.0, 8, 0.5)]
    slots += [("half_opaque", 3, 0.5, 8, 0.5), ("half_through", None, 0.5, 8, 0.5), ("tie_opaque", 5, TIE, 8, 0.5),
              ("tie_through", None, TIE, 8, 0.5), ("short", None, 1.0, 5, 0.5), ("empty", None, 0.5, 0, INF),
              ("marked", None, 1.0, 8, INF), ("stale", 2, 1.0, 8, 0.5), ("through", None, 0.25, 8, 0.5)]
    n_max = len(slots)
    N = n_max + 3
    ids = list(rng.permutation(N)[:n_max])
    R = n_max * n_step
    sig, dl = np.full(R, OPAQUE), np.zeros((R, 2))
    a = rng.integers(4, 11, R)
    # coarse lattices: a sample adds trans * z = 2^-13 * (a multiple of 2^-4) to a running sum of sixteenths
    xyz, feats = _dyadic(rng, -15, 15, 4, (R, 3)), _dyadic(rng, 1, 15, 16, (R, K))
    rays = np.zeros((N, 3), np.int32)
    rays_t = np.full(N, 0.5)
    trans = np.ones(N)
    alive = np.array(ids, np.int32)
    kinds = {}
    for n, (kind, i0, tr, cnt, rt) in enumerate(slots):
        i = int(ids[n])
        s = slice(n * n_step, n * n_step + cnt)
        sig[s] = 0.0
        dl[s, 0] = 2.0 ** -a[s]
        dl[s, 1] = 2.0 ** -(a[s] % 7 + 11)
        if i0 is not None:
            sig[n * n_step + i0] = OPAQUE
        rays[n] = (i, n * n_step, cnt)
        rays_t[i], trans[i] = rt, tr
        kinds[n] = kind
        if kind == "stale":
            rays[n, 0] = int(ids[0])                                              # a row the marcher wrote for another slot
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)
    state = {"weights_sum": rng.integers(1, 8, N) / 16.0, "depth": sign(N) * rng.integers(1, 65, N) / 16.0,
             "image": sign((N, K)) * rng.integers(1, 33, (N, K)) / 16.0, "trans": trans}
    cnt = {"all": n_max, "clipped": n_max + 5, "zero": 0, "negative": -3, "fewer": n_max - 4}[count_kind]
    p = dict(n_alive_max=n_max, n_step=n_step, N=N, K=K, T_thresh=T_thresh, alive_count=cnt, rays_alive=alive, rays_t=rays_t,
             rays=rays, sigmas=sig, feats=feats, deltas=dl, xyzs=xyz, o=_dyadic(rng, -8, 8, 4, (N, 3)),
             d=_dyadic(rng, -8, 8, 4, (N, 3), nonzero=True), **state)
    check_alive_exact(p)
    return p, kinds


def check_alive_exact(p, q=2.0 ** -17):
    """Tier-A conditions of one alive call: trans a power of two >= 2^-13, and for every ray the running sums and every addend
    trans * (a component of z, a feature, 1) on the lattice q with sum |addends| below 2^24 q."""
    n_alive = min(max(int(p["alive_count"]), 0), p["n_alive_max"])
    lt = np.log2(p["trans"])
    assert np.array_equal(lt, np.rint(lt)) and lt.min() >= -13 and lt.max() <= 0
    for n in range(n_alive):
        i, off, cnt = (int(v) for v in p["rays"][n])
        s = slice(off, off + cnt)
        arg = p["sigmas"][s] * p["deltas"][s, 0]
        assert np.all((arg == 0) | (arg >= 1024.0)) and np.all(p["deltas"][s, 0] > 0)
        if not 0 <= i < p["N"] or int(p["rays_alive"][n]) != i:
            continue
        tr = p["trans"][i]
        t = tr * (p["xyzs"][s] - p["o"][i]) * p["d"][i]
        for add, st0 in ((t, p["depth"][i]), (tr * p["feats"][s], p["image"][i]), (np.full((cnt, 1), tr), p["weights_sum"][i])):
            for v in (add, np.atleast_1d(st0)):
                assert np.array_equal(v / q, np.rint(v / q)), "on the lattice"
            assert (np.abs(add).sum(-1).max(initial=0.0) + np.abs(st0).max()) / q < 2.0 ** 24


# ---- lnh_composite_rays (raymarching.cu:966-1053), the RGB template of the alive loop
def rgb_alive_case(n_alive, n_step=4):
    """n_alive rays x two calls.  Kinds by slot: the opaque sample is the LAST of the round (the ray stays alive, saves rays_t and
    dies on the first sample of the next call with weight 0: T = 1 - weights_sum is taken BEFORE the sample), sits earlier (dies
    in the same call), the ray ends with deltas[:, 0] == 0 (dead, rays_t not saved), the ray is transparent (alive, t saved).
    weights_sum starts at 0 or 1/2 with non-zero dyadic running sums."""
    rng = np.random.default_rng(9100 + n_alive)
    kinds = ("opaque_last", "opaque_early", "ends", "through")
    N = n_alive + 2
    ids = rng.permutation(N)[:n_alive].astype(np.int32)
    state = {"weights_sum": np.where(rng.integers(0, 2, N) == 1, 0.5, 0.0), "depth": rng.integers(1, 33, N) / 16.0,
             "image": rng.integers(1, 33, (N, 3)) / 16.0, "rays_t": rng.integers(1, 64, N) / 16.0}
    calls = []
    for call in range(2):
        R = n_alive * n_step
        sig = np.zeros(R)
        a = rng.integers(4, 11, R)
        dl = np.stack([2.0 ** -a, 2.0 ** -(3 + (a - 3 + rng.integers(1, 8, R)) % 8)], 1)
        rgb = _dyadic(rng, 1, 15, 16, (R, 3))
        kind = [kinds[(n + call) % 4] for n in range(n_alive)]
        for n, k in enumerate(kind):
            if k == "opaque_last":
                sig[n * n_step + n_step - 1] = OPAQUE
            elif k == "opaque_early":
                sig[n * n_step + n % (n_step - 1)] = OPAQUE
            elif k == "ends":
                dl[n * n_step + 1 + n % (n_step - 1):(n + 1) * n_step] = 0.0
        calls.append(dict(sigmas=sig, deltas=dl, rgbs=rgb, kind=kind))
    return dict(n_alive=n_alive, n_step=n_step, N=N, ids=ids, state=state, calls=calls)


def rgb_alive_model(n_step, T_thresh, alive, sig, rgb, dl, state, dtype=F):
    """One call of lnh_composite_rays on the first len(alive) slots, as the reference's loop does it, operation by operation."""
    ws, dep, img, rt = (np.array(state[k], dtype) for k in ("weights_sum", "depth", "image", "rays_t"))
    sig, rgb, dl = (np.asarray(a, dtype) for a in (sig, rgb, dl))
    out = np.array(alive, np.int32)
    thr = _thr(T_thresh, dtype)
    for n, i in enumerate(alive):
        t, w_s, d = rt[i], ws[i], dep[i]
        c = img[i].copy()
        step = 0
        while step < n_step:
            r = n * n_step + step
            if dl[r, 0] == 0:
                break
            with np.errstate(under="ignore"):
                alpha = dtype(1) - np.exp(-sig[r] * dl[r, 0])
            T = dtype(1) - w_s
            w = alpha * T
            w_s = w_s + w
            t = t + dl[r, 1]
            d = d + w * t
            c = c + w * rgb[r]
            if T < thr:
                break
            step += 1
        if step < n_step:
            out[n] = -1
        else:
            rt[i] = t
        ws[i], dep[i], img[i] = w_s, d, c
    return {"weights_sum": ws, "depth": dep, "image": img, "rays_t": rt}, out


# ---- lnh_alive_compact
COMPACT_PATTERNS = ("all", "none", "alternating", "wave_first", "wave_last", "trip_first", "trip_last", "list_first", "list_last")


def compact_list(n, pattern):
    """A list of n entries (ray ids >= 0 alive, -1 dead).  wave_* / trip_*: one survivor in EVERY wave / every 1024-trip, at its
    first or last slot (every wave total is 1: the cross-wave prefix counts); list_*: one survivor in the whole list."""
    ids = (np.arange(n) * 7 + 3).astype(np.int32)
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern in ("wave_first", "wave_last", "trip_first", "trip_last"):
        step = 64 if pattern.startswith("wave") else 1024
        keep[(0 if pattern.endswith("first") else step - 1)::step] = True
    elif pattern == "list_first" and n:
        keep[0] = True
    elif pattern == "list_last" and n:
        keep[n - 1] = True
    return np.where(keep, ids, -1).astype(np.int32)


def compact_reference(lst, alive_count, n_alive_max, mistake=None):
    n_in = min(max(int(alive_count), 0), n_alive_max)
    v = np.asarray(lst[:n_in])
    if mistake == "compact_wave_order":            # the wave totals added for the waves BEHIND this one
        out = []
        for base in range(0, n_in, 1024):
            trip = v[base:base + 1024]
            waves = [trip[k:k + 64] for k in range(0, len(trip), 64)]
            for wv in reversed(waves):
                out += [int(x) for x in wv if x >= 0]
        return np.array(out, np.int32), len(out)
    out = v[v >= 0]
    return out.astype(np.int32), len(out)


# ================================================================================================ tier B: inputs
def random_table(N=40, K=2, seed=0, max_count=200, two_surface=10):
    """The random profile of tests/test_occupancy_gpu.py (_ragged: sigma in [0, 30], a tenth of the samples at 2000, unit
    directions, float32 inputs) with counts up to `max_count`, and `two_surface` rays of full length whose background is thin
    (sigma 0.05), whose first surface takes T to about 0.3 and whose second one, 100 samples later, is dense (sigma dt = 30): it lies in the
    next round or the round after.  Rows in arrival order, unowned rows between the rays, a ray that ends at M, one that ends
    at M + 1 (dropped), an empty one."""
    r = np.random.default_rng(seed)
    counts = r.integers(0, max_count + 1, N)
    counts[0], counts[1] = 0, 1
    first = {}
    for k in range(two_surface):
        j = 2 + k
        counts[j] = max_count
        first[j] = 20 + (k * 13) % (max_count - 120)
    order = r.permutation(N)
    drop_j = N - 1
    counts[drop_j] = 33
    last_j = N - 2
    counts[last_j] = max(counts[last_j], min(70, max_count))
    offset = np.zeros(N, np.int64)
    cur = 0
    for j in [j for j in order if j not in (drop_j, last_j)] + [last_j]:
        cur += int(r.integers(0, 3))
        offset[j] = cur
        cur += int(counts[j])
    M = cur
    offset[drop_j] = M + 1 - counts[drop_j]
    R = M + TAIL_ROWS
    sig = (r.random(R) * 30).astype(F)
    sig[r.random(R) < 0.1] = 2000.0
    deltas = np.stack([r.random(R) * 0.02 + 0.002, r.random(R) * 0.03], -1).astype(F)
    for j, s1 in first.items():
        s = slice(offset[j], offset[j] + counts[j])
        sig[s] = 0.05
        sig[offset[j] + s1] = F(1.2 / deltas[offset[j] + s1, 0])                  # T falls to exp(-1.2) = 0.30
        sig[offset[j] + s1 + 100] = F(30.0 / deltas[offset[j] + s1 + 100, 0])
    feats = r.random((R, K)).astype(F)
    o = ((r.random((N, 3)) - 0.5) * 0.2).astype(F)
    d = r.standard_normal((N, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F)
    xyz = np.zeros((R, 3), F)
    index = r.permutation(N)
    for j in range(N):
        t = 0.05 + np.cumsum(r.random(counts[j]) * 0.03)
        xyz[offset[j]:offset[j] + counts[j]] = o[index[j]] + d[index[j]] * t[:, None]
    c = RaggedCase.__new__(RaggedCase)
    c.N, c.K, c.M, c.rows_total = N, K, M, R
    c.count, c.offset, c.index = counts, offset, index
    c.role = ["dropped" if j == drop_j else "last" if j == last_j else "empty" if counts[j] == 0 else "kept" for j in range(N)]
    c.i0 = [None] * N
    c.first_surface = first
    table_order = r.permutation(N)
    c.rays = np.stack([index[table_order], offset[table_order], counts[table_order]], 1).astype(np.int32)
    c.sigma, c.deltas, c.xyz, c.feats, c.o, c.d = sig, deltas, xyz, feats, o, d
    c.g_ws, c.g_depth = r.standard_normal(N).astype(F), (r.standard_normal(N) * 5).astype(F)
    c.g_image = r.standard_normal((N, K)).astype(F)
    return c


TIER_B_SEEDS = ((1, 11), (2, 12), (3, 13))        # (K, seed)
TEETH_PAIRS = ((70, 100), (40, 100), (30, 150))   # (first, second surface): the same round, neighbouring rounds, two apart


def teeth_table(K=2, seed=5):
    """Three two-surface rays of 200 samples with the surfaces at TEETH_PAIRS, float32 inputs."""
    c = random_table(N=len(TEETH_PAIRS) + 4, K=K, seed=seed, two_surface=len(TEETH_PAIRS))
    for k, (s1, s2) in enumerate(TEETH_PAIRS):
        j = 2 + k
        s = slice(c.offset[j], c.offset[j] + c.count[j])
        c.sigma[s] = 0.05
        c.sigma[c.offset[j] + s1] = F(1.2 / c.deltas[c.offset[j] + s1, 0])
        c.sigma[c.offset[j] + s2] = F(30.0 / c.deltas[c.offset[j] + s2, 0])
        c.first_surface[j] = s1
    return c


def old_profile_table(K=2, seed=3):
    """The profile the earlier tests draw: counts below 40 — no ray reaches a second round."""
    return random_table(N=33, K=K, seed=seed, max_count=39, two_surface=0)


# ================================================================================================ tier B: derived bounds
# Standard model: fl(a op b) = (a op b)(1 + d), |d| <= U = 2^-24.  Counted on the kernel text (csrc/transmittance.h
# load_ray_sample, walk_step; csrc/raymarch.hip k_lidar_composite_ragged_fwd / _bwd; csrc/lidar_infer.hip):
#   x = fl(sigma dt)                          1 rounding: exp moves by a relative expm1(|x| gamma(1))
#   e = expf(-x)                              EXPF_ULPS ulp of e (exact at x = 0); below 2^-120 it may be flushed
#   alpha = fl(1 - e)                         at most U alpha and at most e itself (1 is a float)
#   om = fl(1 - alpha)                        U om (no epsilon on the ragged walk)
#   T_{i+1} = Tc incl_i                       a product of i + 1 factors: i roundings inside the scans, in any order, and one
#                                             per round for the carry — i + 1 in all, ONE per sample, whatever the group width
#                                             (the alive compositor's W lanes, its `trans` from call to call: the same chain)
#   w = fl(alpha T)                           1
#   z = fl(fl(fl(fl(x - ox) dx) + fl(fl(y - oy) dy)) + fl(fl(z - oz) dz))     4 on every path: gamma(4) sum |(p - o) d|
#   sums of n terms                           gamma(n) sum |terms| in any order (zeros of idle lanes add exactly)
#   prefix D_i = dc + scan                    i + 1 terms: gamma(i + 1)
#   g_i: (final - prefix) 1, T z 1, their difference 1, times g 1 per channel; gws (1 - ws_final) 2; K + 1 additions; dt 1


def alpha_bounds(sig, dt, E=EXPF_ULPS):
    """float64 x = sigma dt, e = exp(-x), alpha = 1 - e of float32 inputs and the bound of the float32 alpha."""
    sig, dt = np.asarray(sig, np.float64), np.asarray(dt, np.float64)
    x = sig * dt
    with np.errstate(under="ignore"):
        e = np.exp(-x)
    alpha = 1.0 - e
    ulp = np.spacing(np.maximum(e, 2.0 ** -126).astype(F)).astype(np.float64)      # E ulp of the RESULT: 2^-24 just below 1
    d_e = np.where(x == 0, 0.0, e * np.expm1(np.minimum(x * gamma(1), 50.0)) + E * ulp + np.where(e < 2.0 ** -120, e, 0.0))
    d_alpha = np.where(x == 0, 0.0, d_e + np.minimum(U * alpha, e + d_e) + 2.0 ** -53)
    return x, e, alpha, d_alpha


def walk_bounds(sig, dt, T0=1.0, dT0=0.0, E=EXPF_ULPS):
    """float64 walk of one ray from transmittance T0 (known to dT0) and the bounds of alpha, T_i, T_{i+1} (absolute)."""
    x, e, alpha, d_alpha = alpha_bounds(sig, dt, E)
    om = 1.0 - alpha
    d_om = np.where(x == 0, 0.0, d_alpha + U * om + 2.0 ** -53)
    n = len(x)
    T, Tn, dT, dTn = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    t, up = float(T0), float(T0) + float(dT0)
    for i in range(n):
        T[i], dT[i] = t, up - t
        t = t * om[i]
        up = up * (om[i] + d_om[i]) * (1 + U) + TINY
        Tn[i], dTn[i] = t, up - t
    return dict(x=x, e=e, alpha=alpha, om=om, d_alpha=d_alpha, d_om=d_om, T=T, Tn=Tn, dT=dT, dTn=dTn)


def _sum_bound(terms, d_terms, n):
    return d_terms.sum(0) + gamma(n) * (np.abs(terms) + d_terms).sum(0)


def lidar_bounds(c, T_thresh, finals=None, extra_sum_roundings=0, E=EXPF_ULPS):
    """float64 reference of lnh_lidar_composite_rays_train_forward / _backward on float32 inputs and a bound per element.
    Returns the reference arrays, `d_<name>` bounds and `margin`: the smallest |T_{i+1} - T_thresh| / bound(T_{i+1}) over the
    samples up to each ray's stop (the stop DECISION is a comparison of a rounded number).  `finals`: what the backward is
    handed (float32 values; default: the float64 forward)."""
    ref = lidar_reference(c, T_thresh, np.float64, finals)
    N, K, R = c.N, c.K, c.rows_total
    thr = float(F(T_thresh))
    b = {k: np.zeros_like(ref[k]) for k in ("weights_sum", "depth", "image")}
    trans, d_trans = np.ones(N), np.zeros(N)                    # what the alive compositor leaves in `trans`: T behind the last sample that counts
    d_gs, d_gf, A_gs = np.full(R, np.nan), np.full((R, K), np.nan), np.full(R, np.nan)
    wsf, dfin, fin = (np.asarray(a, np.float64) for a in (finals if finals is not None else (ref["weights_sum"], ref["depth"], ref["image"])))
    feats = np.asarray(c.feats, np.float64)
    g_ws, g_d, g_im = (np.asarray(a, np.float64) for a in (c.g_ws, c.g_depth, c.g_image))
    margin = INF
    for index, k in ref["walks"].items():
        s, keep, w, z, last = k["s"], k["keep"], k["w"], k["z"], k["last"]
        n = len(w)
        wb = walk_bounds(c.sigma[s], c.deltas[s, 0], E=E)
        upto = slice(0, last + 1)
        margin = min(margin, float(np.min(np.abs(wb["Tn"][upto] - thr) / wb["dTn"][upto])))
        trans[index], d_trans[index] = wb["Tn"][last], wb["dTn"][last]
        d_w = np.where(keep, wb["d_alpha"] * (wb["T"] + wb["dT"]) + wb["alpha"] * wb["dT"] + U * w + TINY, 0.0)
        d_z = gamma(4) * np.abs(k["t"]).sum(-1)
        f = feats[s]
        d_wz = d_w * (np.abs(z) + d_z) + w * d_z + U * np.abs(w * z) + TINY * keep
        d_wf = d_w[:, None] * f + U * w[:, None] * f + TINY * keep[:, None]
        m = n + extra_sum_roundings
        b["weights_sum"][index] = _sum_bound(w, d_w, m)
        b["depth"][index] = _sum_bound(w * z, d_wz, m)
        b["image"][index] = _sum_bound(w[:, None] * f, d_wf, m)
        # backward
        i1 = np.arange(1, n + 1, dtype=np.float64)
        d_D = np.cumsum(d_wz) + gamma(i1) * np.cumsum(np.abs(w * z) + d_wz)
        d_A = np.cumsum(d_wf, 0) + gamma(i1)[:, None] * np.cumsum(np.abs(w[:, None] * f) + d_wf, 0)
        Tn, dTn = wb["Tn"], wb["dTn"]

        def inner(v, d_v, final, P, d_P):
            a = Tn * v
            d_a = dTn * (np.abs(v) + d_v) + Tn * d_v + U * np.abs(a) + TINY
            q = final - P
            d_q = d_P + U * np.abs(q)
            r = a - q
            return r, d_a + d_q + U * np.abs(r)

        t0 = g_ws[index] * (1.0 - wsf[index])
        terms, d_terms = [np.full(n, t0)], [np.full(n, gamma(2) * abs(t0))]
        r, d_r = inner(z, d_z, dfin[index], k["D"], d_D)
        terms.append(g_d[index] * r)
        d_terms.append(abs(g_d[index]) * d_r + U * np.abs(terms[-1]))
        for ch in range(K):
            r, d_r = inner(f[:, ch], 0.0, fin[index, ch], k["A"][:, ch], d_A[:, ch])
            terms.append(g_im[index, ch] * r)
            d_terms.append(abs(g_im[index, ch]) * d_r + U * np.abs(terms[-1]))
        terms, d_terms = np.stack(terms), np.stack(d_terms)
        d_g = _sum_bound(terms, d_terms, K + 2)
        g = terms.sum(0)
        dt = np.asarray(c.deltas[s, 0], np.float64)
        A_gs[s] = dt * (abs(t0) + abs(g_d[index]) * (Tn * np.abs(z) + abs(dfin[index]) + np.cumsum(np.abs(w * z)))
                        + (np.abs(g_im[index])[None, :] * (Tn[:, None] * f + np.abs(fin[index])[None, :] + np.cumsum(w[:, None] * f, 0))).sum(1))
        d_gs[s] = np.where(keep, dt * d_g + U * np.abs(dt * g) + TINY, np.nan)
        d_gf[s] = np.where(keep[:, None], np.abs(g_im[index])[None, :] * d_w[:, None] + U * np.abs(g_im[index][None, :] * w[:, None]) + TINY, np.nan)
    out = dict(ref)
    out.update({"d_" + k: v for k, v in b.items()})
    out["d_grad_sigmas"], out["d_grad_feats"], out["margin"], out["A_grad_sigmas"] = d_gs, d_gf, margin, A_gs
    out["trans"], out["d_trans"] = trans, d_trans
    return out


def rgb_bounds(c, T_thresh, finals=None, E=EXPF_ULPS):
    """The same for lnh_composite_rays_train_forward / _backward: serial loops, so every sum and product has ONE order; the
    count is the same (T: one rounding per sample; sums and prefixes of i + 1 terms; t = the running sum of deltas[:, 1], i
    roundings; g: three channel terms of 4 roundings, gws (1 - ws_final) 2, three additions, dl0 1).  expf is not pinned and
    alpha is no output of these kernels, so the rest of the chain cannot be separated from it and held exactly: the derived
    bound it is."""
    ref = rgb_reference(c, T_thresh, np.float64, finals)
    N, R = c.N, c.rows_total
    b = {k: np.zeros_like(ref[k]) for k in ("weights_sum", "depth", "image")}
    d_gs, d_gc = np.full(R, np.nan), np.full((R, 3), np.nan)
    wsf, _, fin = (np.asarray(a, np.float64) for a in (finals if finals is not None else (ref["weights_sum"], ref["depth"], ref["image"])))
    rgb = np.asarray(c.feats, np.float64)
    g_ws, g_im = np.asarray(c.g_ws, np.float64), np.asarray(c.g_image, np.float64)
    thr = float(F(T_thresh))
    margin = INF
    for index, k in ref["walks"].items():
        s, keep, w, t = k["s"], k["keep"], k["w"], k["t"]
        n = len(w)
        wb = walk_bounds(c.sigma[s], c.deltas[s, 0], E=E)
        last = int(np.flatnonzero(keep)[-1])
        margin = min(margin, float(np.min(np.abs(wb["Tn"][:last + 1] - thr) / wb["dTn"][:last + 1])))
        d_w = np.where(keep, wb["d_alpha"] * (wb["T"] + wb["dT"]) + wb["alpha"] * wb["dT"] + U * w + TINY, 0.0)
        i1 = np.arange(1, n + 1, dtype=np.float64)
        d_t = gamma(i1) * t
        f = rgb[s]
        d_wt = d_w * (t + d_t) + w * d_t + U * w * t + TINY * keep
        d_wf = d_w[:, None] * f + U * w[:, None] * f + TINY * keep[:, None]
        b["weights_sum"][index] = _sum_bound(w, d_w, n)
        b["depth"][index] = _sum_bound(w * t, d_wt, n)
        b["image"][index] = _sum_bound(w[:, None] * f, d_wf, n)
        d_A = np.cumsum(d_wf, 0) + gamma(i1)[:, None] * np.cumsum(w[:, None] * f + d_wf, 0)
        Tn, dTn = wb["Tn"], wb["dTn"]
        t0 = g_ws[index] * (1.0 - wsf[index])
        terms, d_terms = [np.full(n, t0)], [np.full(n, gamma(2) * abs(t0))]
        for ch in range(3):
            a = Tn * f[:, ch]
            q = fin[index, ch] - k["A"][:, ch]
            r = a - q
            d_r = dTn * f[:, ch] + U * a + TINY + d_A[:, ch] + U * np.abs(q) + U * np.abs(r)
            terms.append(g_im[index, ch] * r)
            d_terms.append(abs(g_im[index, ch]) * d_r + U * np.abs(terms[-1]))
        terms, d_terms = np.stack(terms), np.stack(d_terms)
        d_g = _sum_bound(terms, d_terms, 4)
        dt = np.asarray(c.deltas[s, 0], np.float64)
        d_gs[s] = np.where(keep, dt * d_g + U * np.abs(dt * terms.sum(0)) + TINY, np.nan)
        d_gc[s] = np.where(keep[:, None], np.abs(g_im[index])[None, :] * d_w[:, None] + U * np.abs(g_im[index][None, :] * w[:, None]) + TINY, np.nan)
    out = dict(ref)
    out.update({"d_" + k: v for k, v in b.items()})
    out["d_grad_sigmas"], out["d_grad_rgbs"], out["margin"] = d_gs, d_gc, margin
    return out


# ---- lnh_composite_rays on general alpha: T = 1 - weights_sum, carried from call to call in the state itself
RGB_ALIVE_B = dict(n_alive=40, n_step=8, calls=3, seed=65)   # (a seed with the stop margin below)


def rgb_alive_tier_b(n_alive=40, n_step=8, calls=3, seed=65):
    """The random profile (sigma in [0, 30], a tenth at 2000, float32 inputs) in `calls` rounds of n_step samples per slot; a
    tenth of the slots of a call end early with deltas[:, 0] == 0.  The state starts at zero sums and random rays_t."""
    r = np.random.default_rng(seed)
    N = n_alive + 3
    ids = r.permutation(N)[:n_alive].astype(np.int32)
    state = {"weights_sum": np.zeros(N, F), "depth": np.zeros(N, F), "image": np.zeros((N, 3), F),
             "rays_t": (0.05 + r.random(N)).astype(F)}
    rounds = []
    for _ in range(calls):
        R = n_alive * n_step
        sig = (r.random(R) * 30).astype(F)
        sig[r.random(R) < 0.1] = 2000.0
        dl = np.stack([r.random(R) * 0.02 + 0.002, r.random(R) * 0.03], -1).astype(F)
        for n in np.flatnonzero(r.random(n_alive) < 0.1):
            dl[n * n_step + int(r.integers(1, n_step)):(n + 1) * n_step, 0] = 0.0
        rounds.append(dict(sigmas=sig, deltas=dl, rgbs=r.random((R, 3)).astype(F)))
    return dict(n_alive=n_alive, n_step=n_step, N=N, ids=ids, state=state, calls=rounds)


def rgb_alive_bounds(a, T_thresh, E=EXPF_ULPS):
    """The calls of `a` in float64 (rgb_alive_model, the survivors compacted between the calls) and, per call, a bound for every
    element of the state.  Counted on the loop of k_composite_rays, per sample, with the error of the state carried along:
        alpha                         as everywhere (alpha_bounds)
        T = fl(1 - ws)                the error of ws + U T
        w = fl(alpha T)               1
        ws = fl(ws + w)               = ws (1 - alpha) + alpha: the error of ws times (1 - alpha), the error of alpha times T, the
                                      roundings of T, w and the sum
        t = fl(t + dl1)               + U t
        d = fl(d + fl(w t))           the error of w t (1 rounding) + U d;  the three channels alike
    Returns [(alive list, expected state, bounds, alive list after)] and `margin`: the smallest |T - T_thresh| / bound(T) over
    every sample looked at (the stop test is on a rounded T; deltas[:, 0] == 0 is an exact test)."""
    n_step, thr = a["n_step"], float(F(T_thresh))
    keys = ("weights_sum", "depth", "image", "rays_t")
    state = {k: np.asarray(a["state"][k], np.float64) for k in keys}
    err = {k: np.zeros_like(state[k]) for k in keys}
    alive = [int(i) for i in a["ids"]]
    out, margin = [], INF
    for call in a["calls"]:
        e, after = rgb_alive_model(n_step, T_thresh, alive, call["sigmas"], call["rgbs"], call["deltas"], state, np.float64)
        sig, dl, rgb = (np.asarray(call[k], np.float64) for k in ("sigmas", "deltas", "rgbs"))
        err = {k: v.copy() for k, v in err.items()}
        for n, i in enumerate(alive):
            ws, t, d, c = state["weights_sum"][i], state["rays_t"][i], state["depth"][i], state["image"][i].copy()
            d_ws, d_t, d_d, d_c = err["weights_sum"][i], err["rays_t"][i], err["depth"][i], err["image"][i].copy()
            step = 0
            while step < n_step:
                r = n * n_step + step
                if dl[r, 0] == 0:
                    break
                _, _, alpha, d_alpha = (float(v) for v in alpha_bounds(sig[r], dl[r, 0], E))
                T = 1.0 - ws
                d_T = d_ws + U * abs(T)
                margin = min(margin, abs(T - thr) / d_T if d_T > 0 else INF)
                w = alpha * T
                d_w = d_alpha * (abs(T) + d_T) + alpha * d_T + U * abs(w) + TINY
                ws = ws + w
                # ws + alpha (1 - ws) = ws (1 - alpha) + alpha: the error ws came with is DAMPED by 1 - alpha, not added to
                d_ws = (d_ws * (abs(1.0 - alpha) + d_alpha + U) + d_alpha * abs(T) + (alpha + d_alpha) * U * (abs(T) + d_T)
                        + U * (abs(w) + d_w) + TINY + U * abs(ws))
                t = t + dl[r, 1]
                d_t = d_t + U * abs(t)
                wt = w * t
                d = d + wt
                d_d = d_d + d_w * (abs(t) + d_t) + abs(w) * d_t + U * abs(wt) + TINY + U * abs(d)
                c = c + w * rgb[r]
                d_c = d_c + d_w * rgb[r] + U * np.abs(w * rgb[r]) + TINY + U * np.abs(c)
                if T < thr:
                    break
                step += 1
            if step >= n_step:
                err["rays_t"][i] = d_t
            err["weights_sum"][i], err["depth"][i], err["image"][i] = d_ws, d_d, d_c
            assert ws == e["weights_sum"][i] and d == e["depth"][i], "the bound walks the model's own samples"
        out.append((list(alive), e, err, after))
        state, alive = e, [int(v) for v in after if v >= 0]
    return out, margin


def as_f32_case(c):
    """The tier-B tables already hold float32 values; this asserts it (the references take the inputs as the kernels get them)."""
    for a in (c.sigma, c.deltas, c.xyz, c.feats, c.o, c.d, c.g_ws, c.g_depth, c.g_image):
        assert np.array_equal(np.asarray(a, np.float64), np.asarray(a, F).astype(np.float64))
    return c


@functools.lru_cache(maxsize=None)
def get_tier_b(K, seed):
    return as_f32_case(random_table(K=K, seed=seed))
