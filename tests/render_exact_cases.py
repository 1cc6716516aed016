"""Problems and references of tests/test_render_exact_gpu.py (NumPy only; conditions, coverage and sensitivity are asserted
without a GPU by tests/test_render_exact_cpu.py): the per-ray scan kernels of csrc/lidar_render.hip (lnh_lidar_weights,
lnh_lidar_composite_forward / _backward, lnh_lidar_resample*) and their relatives in csrc/lidar_field.hip
(lnh_lidar_merge_weights, lnh_lidar_sample_points, lnh_lidar_coarse_sample_points).  The walk they share — alpha rule, round of
the product scan, seven-round prefetch — is defined once, in csrc/transmittance.h.

TIER A — one right float32 value in any scan order.  The library is built with -ffp-contract=off and expf is the only operation of
these kernels that IEEE does not pin; the only values of expf every implementation agrees on are expf(-0) = 1 and expf(x) = 0 for
very negative x.  So every sample is TRANSPARENT (sigma = 0: alpha = 0, om = fl(1 + 1e-15) = 1) or OPAQUE (sigma = 2^20 with
delta >= 2^-10: the argument is <= -1024, e = 0, alpha = 1, om = 1e-15f).  Depths lie on the lattice m 2^-10 below 1 with steps out
of {2^-10, 2^-9, 2^-8}, sample_dist is another power of two (or 0 on one ray), density_scale is 1 or 2, colours are n / 16 and the
upstream gradients small integers.  With at most two opaque samples on a ray every weight, sum, prefix and gradient is a two-term
sum or a single product at most (the closed forms of `CompositeCase.expected`), so the carries between 64-sample rounds, between
groups of 7 rounds and between the two passes of the backward are pinned bit for bit.

TIER B — general alpha in (0, 1): float64 references with a bound PER ELEMENT derived from the standard rounding model
(`forward_bounds`, `backward_bounds`, `icdf_bounds`).
"""
import functools

import numpy as np

F = np.float32
U = 2.0 ** -24                 # unit roundoff of float32
EPS = F(1e-15)                 # kTransEps of csrc/transmittance.h
OPAQUE = float(2 ** 20)
ROUND, CHUNKS, WG_RAYS = 64, 7, 4  # (CHUNKS: kChunks of csrc/transmittance.h)
GROUP = ROUND * CHUNKS         # 448 samples are requested at once
LATTICE = 2.0 ** -10

T_SET = (1, 2, 63, 64, 65, 447, 448, 449, 832, 897)
N_SET = (1, 3, 4, 5, 9)
K_SET = (1, 2, 3, 4)
I0_SET = (0, 63, 64, 447, 448, 449)   # and T - 1

# The classic mistakes of such kernels, each applied to the NumPy model below by name (tests/test_render_exact_cpu.py asserts
# that each changes an expected array; the same mistakes compiled into the library all fail tests/test_render_exact_gpu.py).
MISTAKES = ("round_carry", "group_carry", "pref_carry", "last_delta_from_z", "nonlast_delta_from_sd", "break_early",
            "ray_index", "k_stride", "slot_off", "searchsorted_left", "ties_new_first")


# ================================================================================================ tier A: compositing
def ray_patterns(T):
    """(i0, i1) of the rays of length T: first and second opaque sample (None = absent).  i0 at every position class that
    exists (0, 63, 64, 447, 448, 449, T - 1); i1 in the same round, in the next round, in the next group."""
    pats = [(None, None)]
    for i0 in sorted({p for p in I0_SET + (T - 1,) if 0 <= p < T}):
        pats.append((i0, None))
        same = i0 + 1 if (i0 + 1) // ROUND == i0 // ROUND else None
        nxt = (i0 // ROUND + 1) * ROUND + 5
        if nxt >= T:
            nxt = (i0 // ROUND + 1) * ROUND
        grp = (i0 // GROUP + 1) * GROUP + 70
        if grp >= T:
            grp = (i0 // GROUP + 1) * GROUP
        for i1 in (same, nxt, grp):
            if i1 is not None and i1 < T and (i0, i1) not in pats:
                pats.append((i0, i1))
    return pats


def i1_kind(i0, i1):
    kinds = set()
    if i1 // ROUND == i0 // ROUND:
        kinds.add("same round")
    if i1 // ROUND == i0 // ROUND + 1:
        kinds.add("next round")
    if i1 // GROUP == i0 // GROUP + 1:
        kinds.add("next group")
    return kinds


class CompositeCase:
    """N rays of T samples with K colour channels; ray r takes pattern (first + r) of ray_patterns(T)."""

    def __init__(self, N, T, K, density_scale, first=0):
        self.N, self.T, self.K, self.ds = N, T, K, float(density_scale)
        rng = np.random.default_rng(100000 * T + 1000 * N + 10 * K + first)
        pats = ray_patterns(T)
        self.i0, self.i1 = [], []
        zu = np.zeros((N, T), np.int64)
        self.sd = np.zeros(N)
        self.sigma = np.zeros((N, T))
        self.rgb = rng.integers(0, 16, (N, T, K)) / 16.0
        for r in range(N):
            p = first + r
            i0, i1 = pats[p % len(pats)]
            self.i0.append(i0)
            self.i1.append(i1)
            steps = np.ones(max(T - 1, 0), np.int64)
            budget = 1023 - 7 - (T - 1)
            for j in rng.permutation(T - 1)[:max(T // 3, 1)] if T > 1 else []:
                s = int(rng.choice([2, 4]))
                if s - 1 <= budget:
                    steps[j], budget = s, budget - (s - 1)
            z0 = 0 if (i0 == 0 and p % 2 == 1) else int(rng.integers(1, 8))   # z[i0] = 0 shows the second term of depth
            zu[r] = z0 + np.concatenate([[0], np.cumsum(steps)])
            self.sd[r] = 2.0 ** -7 if p % 3 else 2.0 ** -6
            if i0 is not None and i1 is None and i0 < T - 1 and p % 4 == 1:
                self.sd[r] = 0.0                                               # a non-last sample must not take sample_dist
            for i in (i0, i1):
                if i is not None:
                    self.sigma[r, i] = OPAQUE
            if i0 is not None and (p // 2) % 2 == 0:
                self.rgb[r, i0] = 0.0                                          # shows the second term of image
        self.z = zu * LATTICE
        self.g_ws = rng.integers(-8, 9, N).astype(np.float64)
        self.g_depth = rng.integers(-8, 9, N).astype(np.float64)
        self.g_image = rng.integers(-4, 5, (N, K)).astype(np.float64)
        self.perm = np.stack([rng.permutation(T) for _ in range(N)]).astype(np.int32)   # lnh_lidar_merge_weights
        self.sigma_pt = np.zeros((N, T))
        np.put_along_axis(self.sigma_pt, self.perm.astype(np.int64), self.sigma, axis=1)
        self.n_opaque = np.array([(a is not None) + (b is not None) for a, b in zip(self.i0, self.i1)])

    # ---- the upstream gradient of sample i:  c_i = g_ws + g_depth z_i + sum_k g_img_k rgb_ik  (exact in float32 and float64)
    def c(self, null=()):
        g_ws = 0 * self.g_ws if "g_ws" in null else self.g_ws
        g_depth = 0 * self.g_depth if "g_depth" in null else self.g_depth
        g_image = 0 * self.g_image if "g_image" in null else self.g_image
        return g_ws[:, None] + g_depth[:, None] * self.z + (self.rgb * g_image[:, None, :]).sum(-1)

    def deltas(self):
        return np.concatenate([np.diff(self.z, axis=1), self.sd[:, None]], axis=1)

    def expected(self, null=()):
        """The closed forms, computed in float32 where a rounding happens.  NaN in g_sigma = not compared (two opaque
        samples)."""
        N, T, K = self.N, self.T, self.K
        z32, rgb32 = self.z.astype(F), self.rgb.astype(F)
        w = np.zeros((N, T), F)
        ws, depth, image = np.zeros(N, F), np.zeros(N, F), np.zeros((N, K), F)
        for r, (i0, i1) in enumerate(zip(self.i0, self.i1)):
            if i0 is None:
                continue
            w[r, i0], ws[r] = F(1), F(1)
            depth[r], image[r] = z32[r, i0], rgb32[r, i0]
            if i1 is not None:
                w[r, i1] = EPS
                depth[r] = z32[r, i0] + EPS * z32[r, i1]
                image[r] = rgb32[r, i0] + EPS * rgb32[r, i1]
        c, dl = self.c(null), self.deltas()
        gs = np.full((N, T), np.nan)
        for r, (i0, i1) in enumerate(zip(self.i0, self.i1)):
            if i0 is None:
                gs[r] = c[r] * dl[r] * self.ds
            elif i1 is None:
                behind = (EPS * c[r].astype(F)).astype(np.float64)            # fl(1e-15f c_i): the prefix equals `total`
                gs[r] = np.where(np.arange(T) < i0, c[r] - c[r, i0], behind) * dl[r] * self.ds
                gs[r, i0] = 0.0
        g_img32 = (0 * self.g_image if "g_image" in null else self.g_image).astype(F)
        g_rgb = w[:, :, None] * g_img32[:, None, :]
        return {"weights": w, "weights_sum": ws, "depth": depth, "image": image, "g_sigma": gs, "g_rgb": g_rgb,
                "sigma_m": self.sigma.astype(F)}

    def check_conditions(self):
        """The conditions under which the closed forms are the ONE float32 answer."""
        zu = self.z / LATTICE
        assert np.array_equal(zu, np.rint(zu)) and zu.min() >= 0 and self.z.max() < 1.0, "depth lattice"
        if self.T > 1:
            assert set(np.unique(np.diff(zu, axis=1))) <= {1.0, 2.0, 4.0}, "steps are 2^-10, 2^-9 or 2^-8"
        assert set(np.unique(self.sd)) <= {0.0, 2.0 ** -7, 2.0 ** -6}, "sample_dist: a power of two that is no step"
        assert self.ds in (1.0, 2.0)
        assert set(np.unique(self.sigma)) <= {0.0, OPAQUE}
        assert self.n_opaque.max() <= 2, "three opaque samples put a product into the denormal range"
        dl = self.deltas()
        arg = dl * self.ds * self.sigma
        assert np.all((arg == 0) | (arg >= 1024.0)), "expf argument is -0 or <= -1024"
        for r, (i0, i1) in enumerate(zip(self.i0, self.i1)):       # an opaque sample is opaque unless sample_dist = 0 says not
            for i in (i0, i1):
                assert i is None or arg[r, i] >= 1024.0 or (i == self.T - 1 and self.sd[r] == 0.0)
        assert np.array_equal(self.rgb * 16, np.rint(self.rgb * 16)) and self.rgb.min() >= 0 and self.rgb.max() < 1
        for g in (self.g_ws, self.g_depth, self.g_image):
            assert np.array_equal(g, np.rint(g)) and np.abs(g).max() <= 8
        c = self.c()
        assert np.array_equal(c / LATTICE, np.rint(c / LATTICE)) and np.abs(c).max() < 2.0 ** 7
        assert np.array_equal(c.astype(F).astype(np.float64), c)
        assert np.array_equal(np.take_along_axis(self.sigma_pt, self.perm.astype(np.int64), axis=1), self.sigma)


def simulate(c, mistake=None, null=(), merge=False):
    """A float32 model of the kernels' STRUCTURE on a tier-A problem: rounds of 64 with a carried product, groups of 7 rounds,
    the two passes of the backward with `total` and the carried prefix, four rays per workgroup.  Sums are taken in sample order
    (on a tier-A problem every order gives the same bits).  `mistake` names one of MISTAKES; NaN = never written."""
    N, T, K, ds = c.N, c.T, c.K, F(c.ds)
    z, sd, sg = c.z.astype(F), c.sd.astype(F), c.sigma.astype(F)
    rgb = c.rgb.astype(F)
    if merge:
        sg = np.take_along_axis(c.sigma_pt.astype(F), c.perm.astype(np.int64), axis=1)
    if mistake == "k_stride":                                   # sample stride 1, not K
        flat = rgb.reshape(N, T * K)
        rgb = np.stack([flat[:, k:k + T] for k in range(K)], axis=-1)
    g_ws = (0 * c.g_ws if "g_ws" in null else c.g_ws).astype(F)
    g_dp = (0 * c.g_depth if "g_depth" in null else c.g_depth).astype(F)
    g_im = (0 * c.g_image if "g_image" in null else c.g_image).astype(F)
    ci = g_ws[:, None] + g_dp[:, None] * z
    for k in range(K):
        ci = ci + g_im[:, None, k] * rgb[:, :, k]
    n_rounds = -(-T // ROUND)
    run_rounds = n_rounds - 1 if mistake == "break_early" else n_rounds      # (the weights kernel has no such break)
    w = np.full((N, T), np.nan, F)
    gs, g_rgb = np.full((N, T), np.nan, F), np.full((N, T, K), np.nan, F)
    om_all, e_all, dl_all, Ti_all = (np.ones((N, T), F) for _ in range(4))
    ws, dep, img, total = np.zeros(N, F), np.zeros(N, F), np.zeros((N, K), F), np.zeros(N, F)
    carry = np.ones(N, F)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for rd in range(run_rounds):
            if mistake == "group_carry" and rd % CHUNKS == 0:
                carry = np.ones(N, F)
            prod = np.ones(N, F)
            for i in range(rd * ROUND, min(T, (rd + 1) * ROUND)):
                has_next = i + 2 < T if mistake == "nonlast_delta_from_sd" else i + 1 < T
                zn = z[:, i + 1] if i + 1 < T else z[:, i]
                delta = (zn - z[:, i]) if has_next else (np.zeros(N, F) if mistake == "last_delta_from_z" else sd)
                e = np.exp(-delta * ds * sg[:, i]).astype(F)
                alpha = F(1) - e
                om = (F(1) - alpha) + EPS
                Ti = carry * prod
                w[:, i] = alpha * Ti
                om_all[:, i], e_all[:, i], dl_all[:, i], Ti_all[:, i] = om, e, delta, Ti
                ws = ws + w[:, i]
                dep = dep + w[:, i] * z[:, i]
                img = img + w[:, i, None] * rgb[:, i]
                total = total + w[:, i] * ci[:, i]
                prod = prod * om
            if mistake != "round_carry":
                carry = carry * prod
        pref_carry = np.zeros(N, F)
        for rd in range(run_rounds):
            pref = pref_carry.copy()
            for i in range(rd * ROUND, min(T, (rd + 1) * ROUND)):
                pref = pref + w[:, i] * ci[:, i]
                dalpha = Ti_all[:, i] * ci[:, i] - (total - pref) / om_all[:, i]
                gs[:, i] = dalpha * (dl_all[:, i] * ds * e_all[:, i])
                g_rgb[:, i] = w[:, i, None] * g_im
            if mistake != "pref_carry":
                pref_carry = pref
    out = {"weights": w, "weights_sum": ws, "depth": dep, "image": img, "g_sigma": gs, "g_rgb": g_rgb, "sigma_m": sg.copy()}
    if mistake == "ray_index":                                  # two waves share a ray: rays 2 and 3 of a workgroup are never run
        dead = np.arange(N) % WG_RAYS >= 2
        for v in out.values():
            v[dead] = np.nan
    return out


def composite_shapes():
    """(N, T, K, density_scale, first pattern): every T with every K on 9 rays (4 x 9 rays walk through the patterns of that T),
    and the smaller ray counts around the 4 rays of a workgroup."""
    shapes = []
    for T in T_SET:
        for k, K in enumerate(K_SET):
            shapes.append((9, T, K, 1 + (k + T) % 2, 9 * k))
    for N in (1, 3, 4, 5):
        shapes += [(N, 65, 1 + N % 4, 2, 3 * N), (N, 449, 1 + (N + 1) % 4, 1, 5 * N)]
    return shapes


@functools.lru_cache(maxsize=None)
def get_composite_case(N, T, K, ds, first):
    c = CompositeCase(N, T, K, ds, first)
    c.check_conditions()
    return c


def coverage():
    """Position classes met by the composite cases."""
    met = {"i0": set(), "i1": set(), "flags": set(), "T": set(), "N": set(), "K": set(), "ds": set()}
    for shape in composite_shapes():
        c = get_composite_case(*shape)
        met["T"].add(c.T), met["N"].add(c.N), met["K"].add(c.K), met["ds"].add(c.ds)
        for r, (i0, i1) in enumerate(zip(c.i0, c.i1)):
            if i0 is None:
                met["flags"].add("no opaque sample")
                continue
            met["i0"].add("T-1" if i0 == c.T - 1 and i0 not in I0_SET else i0)
            if i0 == c.T - 1:
                met["i0"].add("T-1")
            if i1 is not None:
                met["i1"] |= i1_kind(i0, i1)
            if c.sd[r] == 0.0:
                met["flags"].add("sample_dist = 0")
            if not c.rgb[r, i0].any() and i1 is not None and c.rgb[r, i1].any():
                met["flags"].add("rgb[i0] = 0 with a second opaque sample")
            if c.z[r, i0] == 0.0 and i1 is not None:
                met["flags"].add("z[i0] = 0 with a second opaque sample")
    return met


# ================================================================================================ tier A: sample positions
AABBS = {1.0: np.array([-1.0, -1, -1, 1, 1, 1]), 2.0: np.array([-0.5, -1.5, -0.25, 1.75, 0.5, 1.0])}
POINT_SHAPES = ((1, 1), (3, 85), (4, 64), (1, 257), (5, 13))       # N T = 1, 255, 256, 257 (and several rays)
COARSE_T = (2, 65, 513)                                             # T - 1 a power of two: step * i is exact
COARSE_SHAPES = ((1, 2), (3, 65), (2, 513), (1, 1), (3, 85), (4, 64), (1, 257), (5, 100))


class PointsCase:
    """o = k / 16, d = n / 16, z = m / 256 below 4: o + d z is a multiple of 2^-12 below 2^3, exact in float32, and so are the
    clip and (p + bound) / (2 bound).  Samples leave the box on both sides."""

    def __init__(self, N, T, bound):
        rng = np.random.default_rng(7000 + 100 * N + T + int(bound))
        self.N, self.T, self.bound, self.aabb = N, T, float(bound), AABBS[float(bound)]
        self.o = rng.integers(-12, 13, (N, 3)) / 16.0
        self.d = rng.integers(-16, 17, (N, 3)) / 16.0
        self.z = rng.integers(0, 1024, (N, T)) / 256.0

    def x01(self, z=None):
        p = self.o[:, None, :] + self.d[:, None, :] * (self.z if z is None else z)[..., None]
        for v in (p, (np.clip(p, self.aabb[:3], self.aabb[3:]) + self.bound) / (2 * self.bound)):
            assert np.array_equal(v.astype(F).astype(np.float64), v), "sample positions are exact in float32"
        return (np.clip(p, self.aabb[:3], self.aabb[3:]) + self.bound) / (2 * self.bound)

    def rows(self, T_tot, slot_off, mistake=None):
        """[N, T_tot, 3] with NaN in the rows outside the map."""
        out = np.full((self.N, T_tot, 3), np.nan)
        off = 0 if mistake == "slot_off" else slot_off
        out[:, off:off + self.T] = self.x01()
        return out


def sample_points_f32(o, d, z, aabb, bound):
    """lnh_lidar_sample_points' arithmetic in float32, one rounding per operation (no contraction)."""
    o, d, z, aabb, bound = (np.asarray(a, F) for a in (o, d, z, aabb, bound))
    p = o[:, None, :] + d[:, None, :] * z[..., None]
    p = np.minimum(np.maximum(p, aabb[:3]), aabb[3:])
    return (p + bound) / (F(2) * bound)


def coarse_depths_f32(N, T, near, far, u=None):
    """The stratified depths of csrc/lidar_steps.h in float32, operation by operation."""
    near, far = F(near), F(far)
    i = np.arange(T)
    step = F(1) / F(T - 1) if T > 1 else F(0)
    lin = np.where(i < T // 2, step * i.astype(F), F(1) - step * (T - 1 - i).astype(F)).astype(F)
    t = np.broadcast_to(near + (far - near) * lin, (N, T)).astype(F)
    if u is not None:
        t = t + (np.asarray(u, F) - F(0.5)) * ((far - near) / F(T))
    return t


# ================================================================================================ tier A: resampling
RES_LATTICE = 2.0 ** -14
RES_OPAQUE = float(2 ** 24)
# (N, T, n_new): n_new in {1, 7, 63, 64, 65, 128, 1024} (P = 64, 64, 64, 64, 128, 128, 1024), T in {3, 4, 65, 66, 768}, and the
# call whose dynamic LDS passes 64 KiB
RESAMPLE_SHAPES = ((5, 3, 1), (5, 4, 7), (5, 65, 63), (5, 66, 64), (5, 768, 65), (5, 65, 128), (3, 768, 1024), (5, 4, 1024),
                   (5, 3, 64), (5, 768, 64), (5, 4, 65), (2, 8200, 64))
RESAMPLE_REFUSED = ((1, 2, 64), (1, 768, 0), (1, 768, 1025), (1, 20480, 64))


def padded(n_new):
    P = 64
    while P < n_new:
        P *= 2
    return P


def resample_lds_bytes(T, n_new):
    return 4 * (2 * T + 2 * padded(n_new) + n_new)


class ResampleCase:
    """Rays on the lattice 1 + m 2^-14 (4 + m 2^-14 at T = 8200) with z_0 = z_1 (so z_mid[0] equals both) and ONE opaque sample at T - 2, the last pdf weight:
    nearly all mass sits in the last bin, so u = 1.0 lands on z_mid[T-2] exactly whether the float32 cdf ends at 1 or an ulp
    beside it (lo = nb: below = above, ba - bb = 0; lo = nb - 1: t = 1 - O(u), and t (ba - bb) rounds onto the lattice step).
    u = 0 gives z_mid[0] exactly.  Several j of a ray sit at each end; the rest are generic.  For T <= 4 the pdf has at most two
    terms, the float32 cdf is the same in any order, and EVERY new sample is predicted (`icdf_small`): one u equals cdf[1], which
    separates searchsorted(right) from (left) through the denom < 1e-5 branch of the empty first bin."""

    def __init__(self, N, T, n_new):
        rng = np.random.default_rng(9000 + 7 * T + n_new)
        self.N, self.T, self.n = N, T, n_new
        steps = rng.choice([1, 2, 4], (N, T - 1)) if T <= 768 else np.ones((N, T - 1), np.int64)
        steps[:, 0] = 0                                                    # z_0 = z_1
        # depths in [1, 2) ([4, 8) for the long rays): half an ulp there is more than (ba - bb) delta_cdf of ANY summation order
        self.z = ((2 ** 14 if T <= 768 else 2 ** 16) + rng.integers(1, 8, (N, 1)) + np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(steps, 1)], 1)) * RES_LATTICE
        self.sigma = np.zeros((N, T))
        self.sigma[:, T - 2] = RES_OPAQUE
        self.sd = np.full(N, 2.0 ** -7)
        u = rng.random((N, n_new))
        k = max(1, min(5, n_new // 3))
        self.at0 = np.zeros((N, n_new), bool)
        self.at1 = np.zeros((N, n_new), bool)
        for r in range(N):
            j = rng.permutation(n_new)
            if r % 2 == 0 or n_new > 1:
                self.at0[r, j[:k]] = True
            if n_new >= 2 * k:
                self.at1[r, j[k:2 * k]] = True
            elif r % 2 == 1 and n_new == 1:
                self.at1[r, j[:1]] = True
        u[self.at0], u[self.at1] = 0.0, 1.0
        self.u = u.astype(F)
        if T == 4 and n_new >= 7:                                          # u = cdf[1] of the float32 cdf, bit for bit
            free = ~(self.at0 | self.at1)
            for r in range(N):
                self.u[r, np.flatnonzero(free[r])[0]] = small_cdf(self.z[r], self.sigma[r], self.sd[r])[1]
        self.o = rng.integers(-12, 13, (N, 3)) / 16.0
        self.d = rng.integers(-16, 17, (N, 3)) / 16.0
        self.aabb, self.bound = AABBS[1.0], 1.0

    def z_mid(self):
        return self.z[:, :-1] + 0.5 * np.diff(self.z, axis=1)

    def check_conditions(self):
        zm = self.z_mid()
        assert np.array_equal(zm.astype(F).astype(np.float64), zm) and self.z.min() > 1.0 and self.z.max() < 8.0
        assert np.all(self.z[:, 0] == self.z[:, 1]) and np.all(zm[:, 0] == self.z[:, 0])
        dl = np.diff(self.z, axis=1)
        assert np.all(dl[:, 1:] > 0) and np.all(dl[:, self.T - 2] * RES_OPAQUE >= 1024.0)
        assert self.at0.any() and self.at1.any() and not (self.at0 & self.at1).any()


def small_cdf(z, sigma, sd, ds=1.0):
    """The float32 cdf of a ray with T <= 4 as the kernel forms it: at most two pdf terms, one order."""
    T = len(z)
    assert T in (3, 4)
    z, sg = np.asarray(z, F), np.asarray(sigma, F)
    dl = np.concatenate([np.diff(z), [F(sd)]]).astype(F)
    with np.errstate(under="ignore"):
        e = np.exp(-dl * F(ds) * sg).astype(F)
    alpha = F(1) - e
    om = (F(1) - alpha) + EPS
    Ti = np.concatenate([[F(1)], np.cumprod(om)[:-1]]).astype(F)          # (two or three factors, tier-A values)
    wp = (alpha * Ti)[1:-1] + F(1e-5)
    wsum = wp[0] if T == 3 else wp[0] + wp[1]
    pdf = wp / wsum
    return np.concatenate([[F(0)], np.cumsum(pdf, dtype=F)]).astype(F)


def icdf_small(z, sigma, sd, u, left=False):
    """Every new sample of a ray with T <= 4, in float32 operation by operation (renderer.py:31-44 as the kernel states it)."""
    z, u = np.asarray(z, F), np.asarray(u, F)
    cdf = small_cdf(z, sigma, sd)
    nb = len(z) - 1
    lo = np.searchsorted(cdf, u, side="left" if left else "right")
    below = np.maximum(lo - 1, 0)
    above = np.minimum(lo, nb - 1)
    zm = z[:-1] + F(0.5) * (z[1:] - z[:-1])
    denom = cdf[above] - cdf[below]
    denom = np.where(denom < F(1e-5), F(1), denom)
    t = (u - cdf[below]) / denom
    return zm[below] + t * (zm[above] - zm[below])


def merge_reference(z, new_z, sorted_new, new_first=False):
    """(z_out, perm, new_z out) of the merge of one ray: a stable sort of concat([old, new]) — old first between equal keys,
    then by original index; sorted_new = 1 hands the new samples out in ascending order (slot T + r = r-th smallest key)."""
    z, new_z = np.asarray(z, F), np.asarray(new_z, F)
    T = len(z)
    if sorted_new:
        new_z = np.sort(new_z, kind="stable")
    cat = np.concatenate([z, new_z])
    if new_first:                                                          # the mistake: a new sample goes before an equal old one
        order = np.lexsort((np.arange(len(cat)), np.arange(len(cat)) < T, cat))
    else:
        order = np.argsort(cat, kind="stable")
    return cat[order], order.astype(np.int32), new_z


@functools.lru_cache(maxsize=None)
def get_resample_case(N, T, n_new):
    c = ResampleCase(N, T, n_new)
    c.check_conditions()
    return c


# ================================================================================================ tier B: derived bounds
# Standard model: fl(a op b) = (a op b)(1 + d), |d| <= U = 2^-24; n roundings in a row give at most gamma(n).  expf is good to
# EXPF_ULPS ulp of its result (the one constant neither the code nor IEEE fixes; measured on an MI355X).
EXPF_ULPS = 1.68           # twice the 0.837 ulp measured over 3.9 million arguments in [-87, 0] (1.0 in the denormal range)
TINY = 2.0 ** -126          # a product below the normal range is off by less than this, whether it is kept denormal or flushed
EPS_GAP = abs(float(EPS) - 1e-15)


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _ref64(z, sigma, sd, ds):
    """float64 quantities of renderer.py:233-243 on float32 inputs."""
    z, sigma, sd = (np.asarray(a, np.float64) for a in (z, sigma, sd))
    delta = np.concatenate([np.diff(z, axis=1), sd[:, None] * np.ones_like(z[:, :1])], axis=1)
    x = delta * ds * sigma
    with np.errstate(under="ignore"):
        e = np.exp(-x)
    alpha = 1.0 - e
    om = 1.0 - alpha + 1e-15
    Tr = np.concatenate([np.ones_like(om[:, :1]), np.cumprod(om, axis=1)[:, :-1]], axis=1)
    return delta, x, e, alpha, om, Tr


def forward_bounds(z, sigma, sd, ds, E=EXPF_ULPS):
    """Per-sample bounds |float32 kernel - float64 reference| for alpha, om (relative), the transmittance and the weight.
      * argument: three roundings (z difference, times density_scale, times sigma) move exp by a relative expm1(|x| gamma(3));
        expf adds E ulp = 2 E U relative: eta (0 for a transparent sample: expf(-0) is 1).
      * alpha = fl(1 - e32): error e eta from e, plus the rounding of the subtraction, which is at most U alpha and at most
        e32 itself (1 is a float) — so an exactly opaque sample (e = 0) has NO error in alpha.
      * om = fl(fl(1 - alpha) + 1e-15f): two roundings relative to om, the error of alpha, and |1e-15f - 1e-15|; a transparent
        sample has om32 = 1 against 1 + 1e-15.
      * T_i = prod_{j<i} om_j: the relative errors of the factors and one rounding per scan step (i of them in any order).
        Non-finite once a factor is off by 100 % (a sample so nearly opaque that float32 cannot tell om from 1e-15).
      * w_i = fl(alpha_i T_i)."""
    delta, x, e, alpha, om, Tr = _ref64(z, sigma, sd, ds)
    i = np.arange(z.shape[1], dtype=np.float64)[None, :]
    eta = np.where(x == 0, 0.0, np.expm1(np.minimum(np.abs(x) * gamma(3), 50.0)) + 2 * E * U)     # expf(-0) = 1 on every implementation
    d_alpha = np.where(e == 0, 0.0, e * eta + np.minimum(U * alpha, e * (1 + eta)) + 2.0 ** -53 + 2.0 ** -148)
    r_om = np.where(x == 0, 1e-15, (d_alpha + EPS_GAP) / om + gamma(2))       # alpha = 0: fl(1 + 1e-15f) = 1 against 1 + 1e-15
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        logs = np.where(r_om < 1.0, -np.log1p(-np.minimum(r_om, 0.5)) * (r_om <= 0.5) + np.where(r_om > 0.5, np.inf, 0.0), np.inf)
        L = np.concatenate([np.zeros_like(logs[:, :1]), np.cumsum(logs, axis=1)[:, :-1]], axis=1) - i * np.log1p(-U)
        rho = np.expm1(L)
        d_T = np.where(np.isfinite(rho), Tr * rho, np.inf) + i * TINY
        d_w = (d_alpha * (Tr + d_T) + alpha * d_T) * (1 + U) + U * alpha * Tr + TINY
    return {"delta": delta, "x": x, "e": e, "alpha": alpha, "om": om, "T": Tr, "w": alpha * Tr, "eta": eta, "d_alpha": d_alpha,
            "r_om": r_om, "d_T": d_T, "d_w": d_w}


def sum_bounds(w, d_w, v):
    """Bound of a float32 sum over the samples of fl(w_i v_i) taken in ANY order against sum w_i v_i in float64."""
    T = w.shape[1]
    terms = np.abs(w * v)
    d = d_w * np.abs(v) + U * terms + TINY
    return d.sum(1) + gamma(T) * (terms + d).sum(1)


def backward_bounds(z, sigma, rgb, sd, ds, g_ws, g_depth, g_image, E=EXPF_ULPS, drop=None):
    """float64 g_sigma / g_rgb of the compositing backward (the quotient form, = autograd) and their per-element bounds.
      c_i   K + 1 products and adds: gamma(K + 2) (|g_ws| + |g_depth z| + sum |g_img rgb|)
      w c   fl(w32 c32)
      total, pref_i   sums of T and of i + 1 terms in any order: the errors of the terms + gamma(#terms) sum |w c|
      suffix = fl(total - pref): both errors + one rounding — the part that matters: U (#terms) sum_j |w_j c_j|, absolute
      dalpha = fl(fl(T_i c_i) - fl(suffix / om_i)): the suffix error is divided by om_i
      g_sigma = fl(dalpha fl(fl(delta ds) e_i)).
    `drop` = (ray, i, j): the float64 g_sigma of sample i with w_j c_j left out of its suffix (the teeth of the CPU test)."""
    fb = forward_bounds(z, sigma, sd, ds, E)
    z64, rgb64 = np.asarray(z, np.float64), np.asarray(rgb, np.float64)
    N, T, K = rgb64.shape
    g_ws, g_depth, g_image = (np.asarray(a, np.float64) for a in (g_ws, g_depth, g_image))
    c = g_ws[:, None] + g_depth[:, None] * z64 + (rgb64 * g_image[:, None, :]).sum(-1)
    mag_c = np.abs(g_ws)[:, None] + np.abs(g_depth[:, None] * z64) + np.abs(rgb64 * g_image[:, None, :]).sum(-1)
    d_c = gamma(K + 2) * mag_c
    w, d_w, om, Tr, d_T, e, delta = fb["w"], fb["d_w"], fb["om"], fb["T"], fb["d_T"], fb["e"], fb["delta"]
    wc = w * c
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d_wc = d_w * (np.abs(c) + d_c) + w * d_c + U * np.abs(wc) + TINY
        mag = np.abs(wc) + d_wc
        n = np.arange(1, T + 1, dtype=np.float64)[None, :]
        d_total = d_wc.sum(1, keepdims=True) + gamma(T) * mag.sum(1, keepdims=True)
        d_pref = np.cumsum(d_wc, axis=1) + gamma(n) * np.cumsum(mag, axis=1)
        suffix = np.flip(np.cumsum(np.flip(wc, 1), 1), 1) - wc                 # sum_{j>i} w_j c_j without the cancellation
        if drop is not None:
            r, i, j = drop
            assert j > i
            suffix = suffix.copy()
            suffix[r, i] -= wc[r, j]
        d_suf = (d_total + d_pref) * (1 + U) + U * np.abs(suffix)
        r_om = fb["r_om"]
        q = suffix / om
        d_q = np.where(r_om < 1.0, (d_suf + np.abs(suffix) * r_om) / (om * (1 - np.minimum(r_om, 0.999))), np.inf)
        d_q = d_q * (1 + U) + U * np.abs(q)
        a = Tr * c
        d_a = d_T * (np.abs(c) + d_c) + Tr * d_c + U * np.abs(a) + TINY
        da = a - q
        d_da = (d_a + d_q) * (1 + U) + U * (np.abs(a) + np.abs(q))
        f = delta * ds * e
        d_f = f * (np.expm1(np.log1p(fb["eta"]) + np.log1p(gamma(3))))
        gs = da * f
        d_gs = d_da * (f + d_f) + np.abs(da) * d_f + U * np.abs(gs) + TINY
        d_gs = np.where((f == 0) & (d_f == 0), 0.0, d_gs)                      # exactly opaque: e32 = 0 and the product is 0
        g_rgb = w[:, :, None] * g_image[:, None, :]
        d_grgb = (d_w[:, :, None] + U * w[:, :, None]) * np.abs(g_image[:, None, :]) + TINY
    return {"g_sigma": gs, "d_g_sigma": d_gs, "g_rgb": g_rgb, "d_g_rgb": d_grgb, "c": c, "wc": wc, "fb": fb, "f": f}


def two_surface_rays(N=7, T=832, K=2, seed=21):
    """Rays with a half-transparent first surface around sample 200 and a dense second one around sample 600: float32 inputs.
    The probe pairs of the teeth test sit on them."""
    rng = np.random.default_rng(seed)
    near, far = 0.01, 0.81
    sd = np.full(N, (far - near) / T)
    z = near + (far - near) * np.arange(T)[None, :] / (T - 1) + (rng.random((N, T)) - 0.5) * sd[:, None] * 0.9
    i = np.arange(T)[None, :]
    sigma = 0.5 + 250.0 * np.exp(-((i - 200) / 3.0) ** 2) + 1500.0 * np.exp(-((i - 600) / 4.0) ** 2) * (0.5 + rng.random((N, 1)))
    rgb = rng.random((N, T, K))
    g_ws, g_depth, g_image = 1.0 + rng.random(N), 20.0 + 30.0 * rng.random(N), 0.5 + rng.random((N, K))
    return tuple(a.astype(F) for a in (z, sigma, rgb, sd, g_ws, g_depth, g_image))


# (ray, i, j): inside a round, across a round, across a group, and i well behind the first surface
TEETH_PAIRS = ((0, 195, 200), (1, 190, 200), (2, 440, 600), (3, 300, 600))


# ---- inverse cdf (renderer.py:10-46 as step 1-3 of k_lidar_resample state it)
def icdf_reference(z, sigma, sd, ds, u, E=EXPF_ULPS):
    """float64 new samples of float32 inputs, a bound per sample and the samples left out.
      wp_m = fl(w_{m+1} + 1e-5f): the error of w, one rounding, |1e-5f - 1e-5|
      wsum: nw terms in any order;  pdf_m = fl(wp_m / wsum);  cdf_k: a running sum of k terms — delta_cdf_k grows with its length
      t = fl(fl(u - cb) / denom), denom = fl(ca - cb) or 1 below 1e-5:  (delta_cb + |t| delta_denom) / denom + 3 U |t|; the
      terms under cb are common to ca and cb, so delta_denom holds the error of ONE pdf term and the roundings of both sums
      s = fl(bb + fl(t fl(ba - bb))): delta_t (ba - bb), and two ulp of ba for the midpoints and the last sum (the two z
      differences are exact by Sterbenz: three half-ulp roundings, one of them scaled by (ba - bb) / ba).
    A u within delta_cdf of a knot may fall into the neighbouring bin: the result is continuous there when both bins are regular
    (the larger bound of the two is used) and jumps by a bin when one of them takes the denom < 1e-5 branch — left out, as is a
    sample whose denom lies within its error of 1e-5."""
    fb = forward_bounds(z, sigma, sd, ds, E)
    z64, u64 = np.asarray(z, np.float64), np.asarray(u, np.float64)
    N, T = z64.shape
    nw, nb = T - 2, T - 1
    w, d_w = fb["w"][:, 1:-1], fb["d_w"][:, 1:-1]
    wp = w + 1e-5
    d_wp = d_w + U * wp + abs(float(F(1e-5)) - 1e-5)
    wsum = wp.sum(1, keepdims=True)
    d_wsum = d_wp.sum(1, keepdims=True) + gamma(nw) * (wp + d_wp).sum(1, keepdims=True)
    pdf = wp / wsum
    d_pdf = (d_wp + pdf * d_wsum) / (wsum - d_wsum) + U * pdf
    k = np.arange(1, nw + 1, dtype=np.float64)[None, :]
    cdf = np.concatenate([np.zeros((N, 1)), np.cumsum(pdf, axis=1)], axis=1)                       # [N, nb]
    # delta_cdf_k = D_k + R_k: the errors of its k terms, and the roundings of a running sum of length k (any order)
    D = np.concatenate([np.zeros((N, 1)), np.cumsum(d_pdf, axis=1)], axis=1)
    R = np.concatenate([np.zeros((N, 1)), gamma(k) * np.cumsum(pdf + d_pdf, axis=1)], axis=1)
    d_cdf = D + R
    d_pdf1 = np.concatenate([d_pdf, np.zeros((N, 1))], axis=1)                                     # d_pdf of the bin above knot k
    zm = z64[:, :-1] + 0.5 * np.diff(z64, axis=1)
    s = np.zeros_like(u64)
    bound = np.zeros_like(u64)
    out = np.zeros(u64.shape, bool)

    def one(r, b, a, uu):
        """(s, bound, near the threshold) of bin (b, a) of ray r for the draws uu."""
        cb, ca, bb, ba = cdf[r, b], cdf[r, a], zm[r, b], zm[r, a]
        denom = ca - cb
        d_den = np.where(a > b, d_pdf1[r, b], 0.0) + R[r, a] + R[r, b] + U * denom    # the terms below b are common to both
        near = np.abs(denom - 1e-5) <= d_den + U * 1e-5
        branch = denom < 1e-5
        den = np.where(branch, 1.0, denom)
        d_den = np.where(branch, 0.0, d_den)
        t = (uu - cb) / den
        d_t = (d_cdf[r, b] + U * np.abs(uu - cb) + np.abs(t) * d_den) / (den - d_den) + 2 * U * np.abs(t)
        two_ulp = 2.0 * np.spacing(np.maximum(ba, bb).astype(F)).astype(np.float64)
        return bb + t * (ba - bb), d_t * np.abs(ba - bb) + two_ulp, near, branch

    for r in range(N):
        lo = np.searchsorted(cdf[r], u64[r], side="right")
        below, above = np.maximum(lo - 1, 0), np.minimum(lo, nb - 1)
        s[r], bound[r], near, branch = one(r, below, above, u64[r])
        out[r] = near
        for side in (-1, 1):                                    # the knot under / above u and the bin beyond it
            knot = below if side < 0 else np.minimum(below + 1, nb - 1)
            close = (np.abs(u64[r] - cdf[r, knot]) <= d_cdf[r, knot] + U) & (above > below)
            b2 = np.clip(below + side, 0, nb - 1)
            a2 = np.minimum(b2 + 1, nb - 1)
            s2, bd2, near2, branch2 = one(r, b2, a2, u64[r])
            out[r] |= close & (branch | branch2 | near2)
            bound[r] = np.where(close, np.maximum(bound[r], bd2 + np.abs(s2 - s[r])), bound[r])
    return {"s": s, "bound": bound, "excluded": out, "cdf": cdf, "d_cdf": d_cdf, "z_mid": zm}


STEEP_T = 832


def steep_rays(T=STEEP_T, n_new=64, seed=33):
    """Tier-A weights with one opaque sample at i0 in {1, 62, 63, 64, 65, T - 2}: nearly all mass in one bin, the `run` carry of
    the cdf crossed.  u: half of the draws in the middle half of the first 70 empty bins before the step (the denom < 1e-5 branch;
    further up the ray the derived delta_cdf no longer separates their width 1e-5 / wsum from 1e-5), the rest inside the step; for i0 = 1 there is no empty bin before it and all lie inside."""
    rng = np.random.default_rng(seed)
    i0s = (1, 62, 63, 64, 65, T - 2)
    N = len(i0s)
    steps = rng.choice([1, 2], (N, T - 1))
    z = (rng.integers(1, 8, (N, 1)) + np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(steps, 1)], 1)) * 2.0 ** -11
    sigma = np.zeros((N, T))
    sigma[np.arange(N), i0s] = float(2 ** 21)
    sd = np.full(N, 2.0 ** -7)
    z, sigma, sd = z.astype(F), sigma.astype(F), sd.astype(F)
    cdf = icdf_reference(z, sigma, sd, 1.0, np.zeros((N, 1), F))["cdf"]
    u = np.zeros((N, n_new))
    for r, i0 in enumerate(i0s):
        m = i0 - 1                                               # the step is bin m of the cdf: cdf[m] .. cdf[m + 1]
        top = cdf[r, m + 1] if m + 1 < T - 1 else 1.0
        inside = cdf[r, m] + (0.05 + 0.9 * rng.random(n_new)) * (top - cdf[r, m])
        if m == 0:
            u[r] = inside
            continue
        bins = rng.integers(0, min(m, 70), n_new)                # (far from the 1e-5 threshold in the eyes of the bound too)
        before = cdf[r, bins] + (0.25 + 0.5 * rng.random(n_new)) * (cdf[r, bins + 1] - cdf[r, bins])
        u[r] = np.where(np.arange(n_new) % 2 == 0, before, inside)
    return z, sigma, sd, u.astype(F), i0s


# ---- tier-B inputs shared by the CPU and the GPU file (the random smooth profile of tests/test_lidar_render_gpu.py is torch code)
def _old_profile(*a, **k):
    from test_lidar_render_gpu import _ray_inputs
    return [t.numpy() for t in _ray_inputs(*a, **k)]


def old_profile_backward(K):
    """The case of test_composite_backward_matches_autograd WITHOUT its clamp: ray 0 is empty, ray 1 opaque at its first sample."""
    import torch
    N, T = 29, 832
    z, sigma, rgb, sd = _old_profile(N, T, 2, K)
    g = torch.Generator().manual_seed(5)
    gws, gdp, gim = torch.randn(N, generator=g), torch.randn(N, generator=g) * 50, torch.randn(N, K, generator=g)
    return z, sigma, rgb, sd, gws.numpy(), gdp.numpy(), gim.numpy()


ICDF_CASES = [(d, N, T, n) for d in ("det", "rnd") for N, T, n in ((41, 768, 64), (7, 128, 128), (3, 50, 7))] + ["steep"]


def icdf_inputs(case):
    """(z, sigma, sd, u): the shapes of test_resample_merge with deterministic and random draws, and the steep-bin rays."""
    if case == "steep":
        return steep_rays()[:4]
    import torch
    det, N, T, n = case
    z, sigma, _, sd = _old_profile(N, T, 3)
    if det == "det":
        u = torch.linspace(0.5 / n, 1 - 0.5 / n, n).expand(N, n).contiguous()
    else:
        u = torch.rand(N, n, generator=torch.Generator().manual_seed(4))
    return z, sigma, sd, u.numpy()


def g1_inputs(bins, weights):
    """Kernel inputs that reproduce golden G1 (the reference's own sample_pdf on `bins` [B, 767] and `weights` [B, 766]): a z whose
    midpoints are the bins and, solved in float64, the sigma whose compositing weights are the golden ones — alpha_i = w_i / T_i,
    sigma_i = -log(1 - alpha_i) / delta_i.  Only rows whose weights CAN be compositing weights take part (their sum is at most 1:
    the all-zero row and the one-hot row; the other rows are rand^6 with sums near 109, alpha = w / T would pass 1).  The bins are
    sorted random numbers, so no increasing z has them as midpoints (h_{i+1} = gap_i - h_i must stay inside every gap); z is
    anchored at the sample that carries weight (z_a = b_a - h, z_{a+1} = b_a + h, the recurrence z_{i+1} = 2 b_i - z_i both ways)
    and is NOT monotone elsewhere, where sigma = 0 makes the sign of delta irrelevant.  Steps 0-3 of the kernel, which produce
    new_z, never assume a sorted z.  Returns float32 (z, sigma, sample_dist) and the rows used."""
    bins, weights = np.asarray(bins, np.float64), np.asarray(weights, np.float64)
    rows = np.flatnonzero(weights.sum(1) <= 1.0)
    B, T = len(rows), bins.shape[1] + 1
    z, sigma = np.zeros((B, T)), np.zeros((B, T))
    for k, r in enumerate(rows):
        b, w = bins[r], weights[r]
        a = int(np.argmax(w)) + 1                                # sample a carries weights[a - 1]
        h = 0.25 * min(b[a] - b[a - 1], b[a + 1] - b[a])
        z[k, a] = b[a] - h
        for i in range(a, T - 1):
            z[k, i + 1] = 2 * b[i] - z[k, i]
        for i in range(a - 1, -1, -1):
            z[k, i] = 2 * b[i] - z[k, i + 1]
        Tr = 1.0
        for i in range(1, T - 1):
            if w[i - 1] > 0:
                alpha, delta = w[i - 1] / Tr, z[k, i + 1] - z[k, i]
                assert 0 < alpha <= 1 and delta > 0, "weights that are no compositing weights"
                sigma[k, i] = 2000.0 / delta if alpha == 1 else -np.log1p(-alpha) / delta
                Tr *= 1 - alpha + 1e-15
    return z.astype(F), sigma.astype(F), np.ones(B, F), rows
