"""Problems with a known answer for the occupancy-grid marchers (csrc/raymarch.hip, csrc/lidar_infer.hip over
csrc/march_cell.h), an independent model of the serial walk and a Python emulation of the wave's replay of it.  No GPU.

march_model    the walk of raymarching.cu:331-534, written from march_cell.h and the reference, NOT from oracle/lnh_oracle.c.
               The LATTICE t_{i+1} = fl(t_i + clamp(fl(t_i gamma), dt_min, dt_max)) is float32 (np.float32 scalars) — the one
               float32 formula the model shares with the kernels.  Everything else is exact: positions, levels, cells, Morton
               codes and exits in fractions.Fraction / Python integers over the float32 inputs, the walk on lattice indices.
margins        the float32 kernel and the exact model can decide differently only where a position lies within float32 error of
               a cell face or a level boundary, or a lattice point within that error of an exit.  Every decision of every case
               records (distance to the nearest alternative) / (worst float32 error of the kernel's expression); the CPU file
               asserts the smallest ratio >= 8.  A condition on the INPUTS, not a tolerance on the kernel.
wave_replay    RayWalk::chunk() and the round loop of k_lidar_march_rays over the model's per-lattice-point (valid, occupied,
               exit) values, with named mistakes.  mistake=None must equal the model; every mistake must show.  The mistakes
               exist in this emulator only: no deliberately wrong kernel is built or run (a wrong walk may not terminate).
"""
import math
from fractions import Fraction as Fr

import numpy as np

F = np.float32
MAX_LATTICE = 4096            # lattice points a ray may hold in front of `far` (asserted by the CPU file)
GUARD_LATTICE = 3 * MAX_LATTICE
INF_BITS = 0x7f800000
U = Fr(1, 1 << 24)            # unit roundoff of float32
N_STEPS_LIDAR = (1, 7, 63, 64, 65, 200)
N_STEPS_SERIAL = (1, 64, 300)
SERIAL_KINDS = tuple((k, ns) for k in N_STEPS_SERIAL for ns in (0.0, 0.5))   # the six kinds of call of the serial template

MISTAKES = (
    "pending_dropped",        # `pending` dropped at the chunk boundary
    "skip_resolved",          # a whole-chunk skip treated as resolved
    "ge_includes_pos",        # the `ge` mask of an empty lane includes `pos`
    "run_cut",                # a run cut at the chunk boundary
    "run_mask",               # (1 << run) - 1 taken at run == 64
    "cap_between_chunks",     # the cap tested only between chunks
    "cap_keeps_back",         # the cap keeps the back of a run
    "last_t_not_carried",     # last_t not carried across chunks
    "t_le_far",               # t <= far
    "valid_ignored_pending",  # `valid != ~0` ignored while pending
    "sign0_plus",             # signf(+-0) = +1
    "sign0_zero",             # signf(+-0) = 0
    "level_pos_only",         # the level taken from the position alone
    "no_min_bound",           # min(2^level, bound) dropped
    "lidar_resume_own_t",     # lidar: resume at the last sample's own t
    "lidar_budget",           # lidar: budget ignoring rays_steps
    "lidar_mark",             # lidar: resume mark not +inf when total == max_steps
)
GEOMETRY_MISTAKES = ("sign0_plus", "sign0_zero", "level_pos_only", "no_min_bound")
LIDAR_MISTAKES = ("lidar_resume_own_t", "lidar_budget", "lidar_mark")
# Provably without effect on any output: once a chunk holds a lane with t >= far, every later lane of every later chunk
# does too, so the walk ends at the first `pos` it looks at whatever was pending.  The mistake costs chunks, not samples;
# the emulator counts the chunks it probes and the CPU file holds the mistake to THAT.
OUTPUT_NEUTRAL = ("valid_ignored_pending",)


class Hang(Exception):
    """An iteration guard tripped: on a GPU this walk would not have ended."""


# ================================================================================================ integers
def morton(x, y, z):
    m = 0
    for b in range(10):
        m |= ((x >> b) & 1) << (3 * b) | ((y >> b) & 1) << (3 * b + 1) | ((z >> b) & 1) << (3 * b + 2)
    return m


def _frexp_exponent(x):
    """e with 2^(e-1) <= x < 2^e for a positive Fraction; 0 for 0 (frexpf)."""
    if x == 0:
        return 0
    n, d = x.numerator, x.denominator
    e = n.bit_length() - d.bit_length()
    while (n >= d << e) if e >= 0 else (n << -e >= d):
        e += 1
    while (n < d << (e - 1)) if e >= 1 else (n << (1 - e) < d):
        e -= 1
    return e


def _pow2(x):
    return x > 0 and (x.numerator & (x.numerator - 1)) == 0 and (x.denominator & (x.denominator - 1)) == 0


def _is_f32(x):
    """Is the Fraction a float32 value?"""
    n, d = abs(x.numerator), x.denominator
    if n == 0:
        return True
    if d & (d - 1):
        return False
    return n.bit_length() - ((n & -n).bit_length() - 1) <= 24 and -126 <= n.bit_length() - d.bit_length() <= 126


def _bits(v):
    return int(np.asarray(v, F).view(np.uint32))


# ================================================================================================ grids and cases
class Grid:
    """An occupancy bitfield built bit by bit from (level, (x, y, z)) entries."""

    def __init__(self, H, C, bound, entries, committed_size=True):
        assert H & (H - 1) == 0, "the margin derivation takes H a power of two (k / H and v * H are exact)"
        self.H, self.C, self.bound = H, C, float(bound)
        bits = bytearray(C * H ** 3 // 8)
        for level, (x, y, z) in entries:
            assert 0 <= level < C and all(0 <= c < H for c in (x, y, z))
            i = level * H ** 3 + morton(x, y, z)
            bits[i >> 3] |= 1 << (i & 7)
        self.bits = np.frombuffer(bytes(bits), np.uint8).copy()
        assert not committed_size or 64 <= self.bits.size <= 1536   # (the old profile's H = 128 grid is a CPU-only aside)

    def bit(self, i):
        return (int(self.bits[i >> 3]) >> (i & 7)) & 1


def row(level, axis, c1, c2, pattern):
    """Entries of one row of cells along `axis` ('#' = occupied), the other two cell coordinates (c1, c2) in axis order."""
    out = []
    for k, ch in enumerate(pattern):
        if ch == "#":
            c = [c1, c2]
            c.insert(axis, k)
            out.append((level, tuple(c)))
    return out


class Case:
    def __init__(self, name, grid, max_steps, dt_gamma=0.0):
        self.name, self.grid, self.max_steps, self.dt_gamma = name, grid, max_steps, float(dt_gamma)
        self._rays, self.tags = [], []
        self._model, self._ray_objs, self._derived = {}, {}, {}   # caches: walks / replays, Ray objects, derived cases
        self.cap_override = None                                  # the serial template's n_step in the place of max_steps

    def ray(self, o, d, near, far, noise=0.0, tag=None):
        self._rays.append((tuple(o), tuple(d), near, far, noise))
        self.tags.append(tag)
        return len(self._rays) - 1

    @property
    def N(self):
        return len(self._rays)

    def arrays(self):
        """o [N,3], d [N,3], near, far, noise as float32 (a -0.0 keeps its sign)."""
        o = np.array([r[0] for r in self._rays], F).reshape(-1, 3)
        d = np.array([r[1] for r in self._rays], F).reshape(-1, 3)
        return o, d, np.array([r[2] for r in self._rays], F), np.array([r[3] for r in self._rays], F), \
            np.array([r[4] for r in self._rays], F)

    def derived(self, name, near=None, noise=None, max_cap=None, keep=None):
        """The rays `keep` (all) on the same grid with other start parameters / noise (lidar rounds: noise 0; serial marcher:
        starts from the lattice).  A ray that does not change keeps its cached geometry."""
        c = Case(name, self.grid, self.max_steps, self.dt_gamma)
        for n, (o, d, nr, fr, ns) in enumerate(self._rays):
            if keep is not None and n not in keep:
                continue
            k = c.ray(o, d, nr if near is None else near[n], fr, ns if noise is None else noise[n], self.tags[n])
            if near is None and (noise is None or noise[n] == ns) and n in self._ray_objs:
                c._ray_objs[k] = self._ray_objs[n]
        c.cap_override = max_cap
        return c


# ================================================================================================ the lattice (float32)
class Lattice:
    """t_0 = fl(near + fl(dt(near) noise)), t_{i+1} = fl(t_i + dt(t_i)), dt(t) = fminf(dt_max, fmaxf(dt_min, fl(t gamma)))."""
    _cache = {}

    def __init__(self, near, noise, gamma, max_steps, C, H):
        two_s3 = F(2) * F(1.7320508075688772)
        self.dt_min = two_s3 / F(max_steps)
        self.dt_max = two_s3 * F(1 << (C - 1)) / F(H)
        self.gamma = F(gamma)
        near = F(near)
        self.t = [F(near + F(self.dt(near) * F(noise)))]
        self.q = [Fr(float(self.t[0]))]

    def dt(self, t):
        return min(self.dt_max, max(self.dt_min, F(t * self.gamma)))

    def upto(self, i):
        while len(self.t) <= i:
            if len(self.t) > GUARD_LATTICE:
                raise Hang("lattice guard")
            t = self.t[-1]
            self.t.append(F(t + self.dt(t)))
            self.q.append(Fr(float(self.t[-1])))

    def T(self, i):
        self.upto(i)
        return self.t[i]

    def Q(self, i):
        self.upto(i)
        return self.q[i]

    @classmethod
    def get(cls, near, noise, gamma, max_steps, C, H):
        key = (_bits(near), _bits(noise), _bits(gamma), max_steps, C, H)
        if key not in cls._cache:
            cls._cache[key] = cls(near, noise, gamma, max_steps, C, H)
        return cls._cache[key]


# ================================================================================================ geometry (exact)
class Cell:
    __slots__ = ("i", "gm", "occ", "level", "level_dt", "level_pos", "cell", "clamped", "mb", "p", "eps", "u", "v", "mx")


class Ray:
    """One ray of a case: exact inputs, its lattice, and the exact geometry at lattice points (cached per mistake; the exit
    and the margins are worked out only where somebody asks for them)."""

    def __init__(self, case, n):
        o, d, near, far, noise = case._rays[n]
        g = case.grid
        self.case, self.n, self.g = case, n, g
        self.o = [Fr(float(F(v))) for v in o]
        self.d32 = [F(v) for v in d]
        self.d = [Fr(float(v)) for v in self.d32]
        self.neg0 = [bool(np.signbit(v)) for v in self.d32]
        self.has_zero = any(v == 0 for v in self.d)
        self.far = F(far)
        self.lat = Lattice.get(near, noise, case.dt_gamma, case.max_steps, g.C, g.H)
        self.bound = Fr(g.bound)
        self._geo, self._exit, self._const, self._margin, self._mb = {}, {}, {}, {}, {}
        n_valid = 0
        while self.lat.T(n_valid) < self.far:      # (False at once for a NaN far)
            n_valid += 1
            if n_valid > MAX_LATTICE:
                raise Hang(f"{case.name} ray {n}: more than {MAX_LATTICE} lattice points in front of far")
        self.n_valid = n_valid

    def valid(self, i, mistake=None):
        if mistake == "t_le_far":
            return bool(self.lat.T(i) <= self.far)
        return i < self.n_valid

    def geo(self, i, gm=None):
        if gm in ("sign0_plus", "sign0_zero"):
            gm = None                                 # the sign of a zero only enters the exit
        key = (i, gm)
        c = self._geo.get(key)
        if c is None:
            c = self._geo[key] = self._probe(i, gm)
        return c

    def _probe(self, i, gm):
        g, B, H = self.g, self.bound, self.g.H
        if gm is not None:
            b = self.geo(i)
            level = b.level_pos if gm == "level_pos_only" else b.level
            mb = Fr(2) ** level if gm == "no_min_bound" else min(Fr(2) ** level, B)
            if level == b.level and mb == b.mb:
                return b                              # the mistake changes nothing at this point
            c = Cell()
            c.i, c.gm, c.p, c.eps, c.clamped, c.level_pos, c.level_dt, c.v, c.mx = i, gm, b.p, b.eps, b.clamped, b.level_pos, b.level_dt, b.v, b.mx
        else:
            t, dt = self.lat.Q(i), Fr(float(self.lat.dt(self.lat.T(i))))
            raw = [self.o[a] + t * self.d[a] if self.d[a] else self.o[a] for a in range(3)]
            c = Cell()
            c.i, c.gm = i, None
            c.p = [min(B, max(-B, x)) for x in raw]
            c.eps = raw                               # (the error of fmaf(t, d, o) is worked out from this in margin())
            c.clamped = [abs(x) > B for x in raw]
            c.mx = max(abs(x) for x in c.p)
            c.v = dt * H / 2
            c.level_pos = min(g.C - 1, max(0, _frexp_exponent(c.mx))) if g.C > 1 else 0
            c.level_dt = min(g.C - 1, max(0, _frexp_exponent(c.v))) if g.C > 1 else 0
            level = max(c.level_pos, c.level_dt)
            mb = min(Fr(2) ** level, B)
        c.level, c.mb = level, mb
        c.u = [self._coord(a, c.p[a], mb) for a in range(3)]
        c.cell = [min(H - 1, max(0, math.floor(x[0]))) for x in c.u]
        c.occ = bool(g.bit(level * H ** 3 + morton(*c.cell)))
        return c

    def _coord(self, a, x, mb):
        """The exact cell coordinate (x / mip_bound + 1) / 2 * H of axis a, the worst error of its float32 evaluation at zero
        position error, and its distance to the nearest cell face (a component the ray does not move along is worked out
        once per mip_bound)."""
        key = (a, mb) if self.d[a] == 0 else None
        if key is not None and key in self._const:
            return self._const[key]
        H = self.g.H
        k = self._mb.get(mb)
        if k is None:
            k = self._mb[mb] = (Fr(H, 2) / mb, Fr(H, 2), 0 if _pow2(mb) else U)   # scale, H / 2, error of fl(1 / mip_bound)
        scale, half, d_r = k
        u = x * scale + half
        # fmaf(x, rbound, 1) lies in [0, 2] and is u * 2 / H: exact where that is a float32 and rbound is exact
        err = half * (abs(x) / mb * d_r + U) if d_r else (0 if _is_f32(u) else half * U)
        f = round(u)
        got = (u, err, abs(u - (1 if f < 1 else H - 1 if f > H - 1 else f)))
        if key is not None:
            self._const[key] = got
        return got

    def _eps(self, c):
        """float32 error of fmaf(t, d, o) behind the clamp: none where the exact value is a float32 or lies beyond the bound."""
        out = []
        for a, x in enumerate(c.eps):
            if self.d[a] == 0:
                out.append(0)
                continue
            e = 0 if _is_f32(x) else U * abs(x)
            out.append(0 if abs(x) - e >= self.bound else e)
        return out

    def margin(self, i):
        """The kernel's float32 decisions at lattice point i (march_cell.h), as distance / worst error: the smallest."""
        if i not in self._margin:
            self._margin[i] = self._margin_of(i)
        return self._margin[i]

    def _margin_of(self, i):
        c, g, H = self.geo(i), self.g, self.g.H
        eps = self._eps(c)
        ratio = math.inf
        for k in range(g.C - 1):                     # level boundaries 2^k that separate two levels
            ratio = min(ratio, _ratio(abs(c.mx - Fr(2) ** k), max(eps)))
            # fl(dt * H), then * 0.5 exactly: one rounding unless the product is a float32 (always, for H a power of two)
            ratio = min(ratio, _ratio(abs(c.v - Fr(2) ** k), 0 if _is_f32(c.v) else U * c.v))
        for a in range(3):
            _, err, dist = c.u[a]
            if eps[a] != 0:                          # an inexact position: its error, and fmaf rounds whatever the sum is
                d_r = 0 if _pow2(c.mb) else U
                err = Fr(H, 2) * (eps[a] / c.mb + abs(c.p[a]) / c.mb * d_r + U)
            ratio = min(ratio, _ratio(dist, err))
        return ratio

    def exit(self, i, gm=None, with_error=False):
        """The exact parameter at which the ray leaves the (empty) cell of lattice point i, over the axes with d != 0;
        with_error: and the worst float32 error of the kernel's tt."""
        if not self.has_zero and gm in ("sign0_plus", "sign0_zero"):
            gm = None
        key = (i, gm)
        if key not in self._exit:
            self._exit[key] = self._exit_of(i, gm)
        ex, err = self._exit[key]
        return (ex, err) if with_error else ex

    def _exit_of(self, i, gm):
        c, H = self.geo(i, gm), self.g.H
        t = self.lat.Q(i)
        eps = self._eps(c) if gm is None else [0] * 3
        best, taus = None, []
        for a in range(3):
            zero = self.d[a] == 0
            if zero and gm not in ("sign0_plus", "sign0_zero"):
                continue                              # (F - x) * (+-inf) = +inf, or NaN on the face: fminf passes it over
            if zero:
                # the mistaken sign of a zero: which face, and the sign of (F - x) * rd with rd = +-inf
                k = c.cell[a] + 1 if gm == "sign0_plus" else Fr(2 * c.cell[a] + 1, 2)
                diff = (Fr(2) * k / H - 1) * c.mb - c.p[a]
                if diff != 0 and (diff > 0) == self.neg0[a]:
                    best = Fr(-1)                     # -inf: the exit collapses to t
                continue
            k = c.cell[a] + (1 if self.d[a] > 0 else 0)
            tau = ((Fr(2 * k, H) - 1) * c.mb - c.p[a]) / self.d[a]
            taus.append((tau, eps[a] / abs(self.d[a]) + 3 * U * abs(tau)))   # F - x, 1 / d, the product
            best = tau if best is None else min(best, tau)
        assert taus, "a zero direction has no exit (and no end in the reference either)"
        ex = t + max(Fr(0), best)
        tmin, emin = min(taus)
        return ex, max(e for tau, e in taus if tau - e <= tmin + emin) + U * abs(ex)   # + the sum t + tau


def _ratio(dist, err):
    if err == 0:
        return math.inf                               # the kernel's value is the exact one: no margin is needed
    return float(dist / err)


# ================================================================================================ the model
class Walk:
    """What the model says about one ray."""

    def __init__(self):
        self.idx, self.empties, self.levels, self.visited = [], [], [], []
        self.end, self.ratio = None, math.inf


def _jump(ray, i, ex):
    """First j > i with t_j >= ex (as a lattice index; indices >= n_valid are in front of nothing)."""
    j = i + 1
    while ray.lat.Q(j) < ex:
        j += 1
        if j > GUARD_LATTICE:
            raise Hang("jump guard")
    return j


def model_ray(case, n, cap=None, margins=False):
    ray = case_ray(case, n)
    cap = case.max_steps if cap is None else cap
    w = Walk()
    i = guard = 0
    while True:
        guard += 1
        if guard > 4 * MAX_LATTICE:
            raise Hang(f"{case.name} ray {n}: model guard")
        if i >= ray.n_valid:
            w.end = "far"
            break
        if len(w.idx) >= cap:
            w.end = "cap"
            break
        c = ray.geo(i)
        if margins:
            w.ratio = min(w.ratio, ray.margin(i))
        w.levels.append(c.level)
        w.visited.append(i)
        if c.occ:
            w.idx.append(i)
            i += 1
        else:
            ex, err = ray.exit(i, with_error=True)
            j = _jump(ray, i, ex)
            if margins:
                dist = ray.lat.Q(j) - ex
                if j - 1 > i:
                    dist = min(dist, ex - ray.lat.Q(j - 1))
                w.ratio = min(w.ratio, _ratio(dist, err))
            w.empties.append((i, j))
            i = j
    w.stop_index = i
    if not margins:
        w.ratio = None
    return w


def case_ray(case, n):
    rays = case._ray_objs
    if n not in rays:
        rays[n] = Ray(case, n)
    return rays[n]


def march_model(case, cap=None, margins=False):
    """Per ray: the Walk (emitted lattice indices and bookkeeping).  Cached.  margins: also the smallest margin ratio of the
    ray's decisions (Walk.ratio; None without) — the CPU file asks for them, the GPU file has no use for them."""
    cap = case.cap_override if cap is None else cap
    if ("model", cap, True) in case._model:
        return case._model[("model", cap, True)]
    key = ("model", cap, margins)
    if key not in case._model:
        case._model[key] = [model_ray(case, n, cap, margins) for n in range(case.N)]
    return case._model[key]


def expected_rows(case, n, idx):
    """deltas [k, 2] and the lattice parameters of the samples `idx` of ray n, as float32:
    deltas[:, 0] = dt_i, deltas[:, 1] = fl(t_{i+1} - t after the previous sample) (t_0 in front of the first)."""
    lat = case_ray(case, n).lat
    out = np.zeros((len(idx), 2), F)
    prev = lat.T(0)
    for k, i in enumerate(idx):
        out[k, 0] = lat.dt(lat.T(i))
        out[k, 1] = F(lat.T(i + 1) - prev)
        prev = lat.T(i + 1)
    return out


def xyz_is_correctly_rounded(case, n, idx, xyz):
    """xyzs as a condition: each float32 must be a correctly rounded clip(o + t d): 2 |x - exact| <= spacing(x)."""
    ray = case_ray(case, n)
    xyz = np.asarray(xyz, F)
    if not np.isfinite(xyz).all():
        return False
    for k, i in enumerate(idx):
        exact = ray.geo(i).p
        for a in range(3):
            x = F(xyz[k, a])
            if Fr(float(x)) == exact[a]:
                continue
            beyond = np.nextafter(x, F(np.inf) if exact[a] > Fr(float(x)) else F(-np.inf))   # the neighbour on the exact value's side
            if 2 * abs(Fr(float(x)) - exact[a]) > abs(Fr(float(beyond)) - Fr(float(x))):
                return False
    return True


def lidar_rounds_model(case, n_step):
    """The alive loop from the model's samples: a list of rounds, each {ray id: (count, first sample, rays_t bits, total)},
    for the rays alive in it (rays_t != +inf), in id order."""
    walks = march_model(case)
    done = [0] * case.N
    alive = list(range(case.N))
    rounds = []
    while alive:
        rnd = {}
        for n in alive:
            idx = walks[n].idx
            take = min(n_step, len(idx) - done[n])
            total = done[n] + take
            if take == n_step and total < case.max_steps:
                mark = _bits(case_ray(case, n).lat.T(idx[total - 1] + 1))
            else:
                mark = INF_BITS
            rnd[n] = (take, done[n], mark, total)
            done[n] = total
        rounds.append(rnd)
        alive = [n for n in alive if rnd[n][2] != INF_BITS]
        assert len(rounds) <= case.max_steps // n_step + 2
    return rounds


# ================================================================================================ the wave emulator
def _chunk(ray, base, st, cap, m):
    """RayWalk::chunk over lattice points base .. base + 63.  st: pending, tt, emitted, done, last (lattice index after the
    last sample), chunks.  Returns the emitted lattice indices."""
    gm = m if m in GEOMETRY_MISTAKES else None
    st["chunks"] += 1
    if st["chunks"] > 4 * MAX_LATTICE // 64:
        raise Hang("chunk guard")
    if m == "t_le_far":
        flags = [ray.valid(base + k, m) for k in range(64)]
        valid, all_valid = flags.__getitem__, all(flags)
    else:                                             # t grows along the lanes: the valid lanes are a prefix
        valid, all_valid = (lambda k: base + k < ray.n_valid), base + 63 < ray.n_valid
    occ = lambda k: valid(k) and ray.geo(base + k, gm).occ
    emit, pos = [], 0
    if m == "pending_dropped":
        st["pending"] = False
    if st["pending"]:
        ge = next((k for k in range(64) if ray.lat.Q(base + k) >= st["tt"]), None)
        if ge is None:
            if m == "skip_resolved":
                st["pending"] = False
            if not all_valid and m != "valid_ignored_pending":
                st["done"] = True
            return emit
        pos, st["pending"] = ge, False
    spins = 0
    while pos < 64:
        spins += 1
        if spins > 200:
            raise Hang("the lane loop spins")
        if not valid(pos):
            st["done"] = True
            break
        if st["emitted"] + (0 if m == "cap_between_chunks" else len(emit)) >= cap:
            st["done"] = True
            break
        if occ(pos):
            run = 0
            while pos + run < 64 and occ(pos + run):
                run += 1
            if not (m == "run_mask" and run >= 64):               # (1 << 64) - 1 = 0 on the hardware's shifter
                emit += range(pos, pos + run)
            pos += run
            if m == "run_cut" and pos == 64:
                st["done"] = True
        else:
            tt = ray.exit(base + pos, gm)
            first = pos if m == "ge_includes_pos" else pos + 1
            ge = next((k for k in range(first, 64) if ray.lat.Q(base + k) >= tt), None)
            if ge is None:
                st["pending"], st["tt"] = True, tt
                break
            pos = ge
    if m != "cap_between_chunks":
        while st["emitted"] + len(emit) > cap:
            emit.pop(0 if m == "cap_keeps_back" else -1)
            st["done"] = True
    if not all_valid:
        st["done"] = True
    return [base + k for k in emit]


def _walk(ray, start, cap, m, lidar=False):
    """Chunks from lattice index `start` until done (training) or until the budget is used up (lidar).  Returns the
    emitted indices, deltas[:, 1] as bits, the chunk count."""
    lat = ray.lat
    st = dict(pending=False, tt=None, emitted=0, done=cap == 0 and lidar, chunks=0)
    idx, d1, base, last = [], [], start, lat.T(start)
    while not st["done"]:
        em = _chunk(ray, base, st, cap, m)
        base += 64
        for k, i in enumerate(em):
            d1.append(_bits(F(lat.T(i + 1) - (lat.T(em[k - 1] + 1) if k else last))))
        if em:
            if m != "last_t_not_carried":
                last = lat.T(em[-1] + 1)
            idx += em
            st["emitted"] += len(em)
        if lidar and st["emitted"] >= cap:
            break
    return idx, d1, st["chunks"]


def wave_replay(case, mistake=None, n_step=None):
    """n_step None: the training walk — per ray (indices, deltas[:, 1] bits, chunks).
    n_step k: the alive loop of k_lidar_march_rays in rounds of k — the rounds in the shape of lidar_rounds_model, the
    samples as lists of lattice indices: {ray: (indices, rays_t bits, rays_steps)}.
    A walk that trips a guard is reported as the string "hang"."""
    key = ("replay", mistake, n_step)
    if key not in case._model:
        case._model[key] = _wave_replay(case, mistake, n_step)
    return case._model[key]


def _wave_replay(case, m, n_step):
    if n_step is None:
        out = []
        for n in range(case.N):
            try:
                out.append(_walk(case_ray(case, n), 0, case.max_steps, m))
            except Hang:
                out.append("hang")
        return out
    rays_t = [0] * case.N                    # the resume parameter as a lattice index; None = +inf
    steps = [0] * case.N
    alive, rounds = list(range(case.N)), []
    while alive:
        rnd = {}
        for n in alive:
            ray = case_ray(case, n)
            before = min(steps[n], case.max_steps)
            budget = min(n_step, case.max_steps if m == "lidar_budget" else case.max_steps - before)
            try:
                idx, _, _ = _walk(ray, rays_t[n], budget, m, lidar=True)
            except Hang:
                return "hang"
            total = before + len(idx)
            steps[n] = total
            go_on = len(idx) == n_step and (total < case.max_steps or m == "lidar_mark")
            rays_t[n] = (idx[-1] if m == "lidar_resume_own_t" else idx[-1] + 1) if go_on else None
            rnd[n] = (idx, _bits(ray.lat.T(rays_t[n])) if go_on else INF_BITS, total)
        rounds.append(rnd)
        alive = [n for n in alive if rnd[n][1] != INF_BITS]
        if len(rounds) > case.max_steps // n_step + 4:
            return "hang"
    return rounds


def model_as_replay(case, n_step=None):
    """The model's answer in the shape wave_replay returns (without the chunk count)."""
    walks = march_model(case)
    if n_step is None:
        return [(w.idx, [_bits(v) for v in expected_rows(case, n, w.idx)[:, 1]]) for n, w in enumerate(walks)]
    return [{n: (walks[n].idx[first:first + take], mark, total) for n, (take, first, mark, total) in rnd.items()}
            for rnd in lidar_rounds_model(case, n_step)]


# ================================================================================================ the cases
def _dt(max_steps):
    return float(F(2) * F(1.7320508075688772) / F(max_steps))


def _near_for(face_t, j, dt, q=1024):
    """A dyadic near that puts lattice index j first behind the parameter face_t (constant dt, noise 0)."""
    return round((face_t - (j - 0.5) * dt) * q) / q


def _axis_lattice(near, max_steps, n):
    """float32 lattice of constant dt by sequential accumulation (for choosing phases; the tests judge the result)."""
    return np.add.accumulate(np.concatenate([[F(near)], np.full(n, F(_dt(max_steps)), F)]), dtype=F)


AXIS_ZEROS = ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0))
PATTERNS8 = ("........", "########", ".#......", "#.......", ".......#", "#.#.#.#.", ".##.....", "..####..",
             "#......#", ".#.#....", "##.....#", "...#....", "....##..", ".######.", "#.##.###", "..#.....")


def _centre(cell, H, mb=1.0):
    return ((cell + 0.5) / H * 2 - 1) * mb


def _case_rows8():
    """H = 8, C = 1, bound 1, max_steps 1024: 16 rows along x, each with its own pattern, walked from six phases; the
    constructed phases (exits on lane 0 / 63, a run that ends on lane 63, a whole-chunk skip); the far events."""
    H, dt = 8, _dt(1024)
    entries = []
    for p, pat in enumerate(PATTERNS8):
        entries += row(0, 0, p % 8, p // 8, pat)
    c = Case("rows8", Grid(H, 1, 1.0, entries), 1024)
    where = lambda p: (_centre(p % 8, H), _centre(p // 8, H))
    for p in range(len(PATTERNS8)):
        y, z = where(p)
        for k, far in ((3, 1.96875 if p < 10 else 0.84375), (37, 0.59375), (100, 0.34375)):
            c.ray((-1.0, y, z), (1.0, 0.0, 0.0), k / 1024, far)
    y, z = where(2)                                   # ".#......": the first point is empty, the exit at t = 0.25
    for j in (64, 63, 127, 128):
        c.ray((-1.0, y, z), (1.0, 0.0, 0.0), _near_for(0.25, j, dt), 1.96875, tag=f"exit_lane_{j % 64}")
    y, z = where(3)                                   # "#.......": a run of exactly lanes 0 .. 63
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), _near_for(0.25, 64, dt), 1.96875, tag="run_0_63")
    near = _near_for(0.25, 64, dt)
    ts = _axis_lattice(near, 1024, 200)
    for tag, far in (("far_eq", ts[64]), ("far_below", np.nextafter(ts[64], F(0))), ("far_above", np.nextafter(ts[64], F(9))),
                     ("far_eq", ts[40]), ("far_below", np.nextafter(ts[40], F(0))), ("far_above", np.nextafter(ts[40], F(9)))):
        c.ray((-1.0, where(1)[0], where(1)[1]), (1.0, 0.0, 0.0), near, float(far), tag=tag)   # the full row
    y, z = where(5)                                   # "#.#.#.#.": met at lane ~60 of chunk 0, exit in chunk 2
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), _near_for(0.25, 60, dt), 1.96875, tag="skip_one_chunk")
    y, z = where(3)                                   # "#.......": far inside the pending empty cell, two chunks on
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), 3 / 1024, 0.45, tag="far_in_pending")
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), 3 / 1024, 0.28, tag="far_in_empty")
    y, z = where(1)
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), 0.5, 0.25, tag="far_lt_near")
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), 0.5, float("nan"), tag="far_nan")
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), 3 / 1024, 2.9375, tag="clamped")          # behind the box: the cell stays H - 1
    y, z = where(0)
    c.ray((-1.0, y, z), (1.0, 0.0, 0.0), 1.75, 2.25, tag="clamped_empty")         # ... and empty: exit = t, one point a time
    for ns in (0.5, float(np.nextafter(F(1), F(0)))):
        for p in (1, 5, 9):
            c.ray((-1.0,) + where(p), (1.0, 0.0, 0.0), 20 / 1024, 1.96875, noise=ns)
    return c


def _case_axes():
    """The six axis directions, each with its zero components as (+0, +0), (-0, -0), (+0, -0), through cell centres and
    through points a quarter cell off them; plane-parallel rays; directions that are no unit vectors.  H = 8, C = 1."""
    H = 8
    entries = []
    for axis in range(3):
        for k, pat in enumerate(("#.##..#.", ".#...##.", "##....##")):
            entries += row(0, axis, 2 + k, 5 - k if axis != 1 else 6 - k, pat)
    entries += [(0, (x, y, 3)) for x in range(8) for y in range(8) if (x + 2 * y) % 3 != 1]      # a plane for the diagonals
    c = Case("axes", Grid(H, 1, 1.0, entries), 1024)
    for axis in range(3):
        for s in (1.0, -1.0):
            for k in range(3):
                c1, c2 = 2 + k, (5 - k if axis != 1 else 6 - k)
                for off in (0.0, 1 / 16):
                    for zi, (z0, z1) in enumerate(AXIS_ZEROS):
                        o = [_centre(c1, H) + off, _centre(c2, H) - off]
                        o.insert(axis, -s * 1.0)
                        d = [z0, z1]
                        d.insert(axis, s * (1.0 if off == 0 else 2.0))
                        if off and k:
                            continue
                        c.ray(o, d, 5 / 1024, (1.96875 if zi == k % 3 and not off and k == 0 else 0.34375) / abs(d[axis]))
    zc = _centre(3, H)
    for dx, dy in ((1.0, 0.5), (-1.0, 0.75), (0.5, -1.0), (-0.25, -1.0), (3.0, 1.0), (-1.0, 2.0)):   # plane-parallel, |d| != 1
        for z0 in (0.0, -0.0):
            o = (-0.9375 * np.sign(dx), -0.90625 * np.sign(dy), zc + 1 / 32)
            c.ray(o, (dx, dy, z0), 3 / 1024, 1.75 / max(abs(dx), abs(dy)))
    return c


def _case_rows2048():
    """max_steps = 2048: 148 lattice points per level-0 cell, an empty cell met in chunk c with its exit in chunk c + 3."""
    H, dt = 8, _dt(2048)
    pats = ("#.#.....", ".#......", "..#.....", "#..#....")
    entries = []
    for p, pat in enumerate(pats):
        entries += row(0, 0, p, 7 - p, pat)
    c = Case("rows2048", Grid(H, 1, 1.0, entries), 2048)
    for p in range(len(pats)):
        y, z = _centre(p, H), _centre(7 - p, H)
        for near in (_near_for(0.25, 60, dt, 2048), _near_for(0.25, 128, dt, 2048), 7 / 2048):
            c.ray((-1.0, y, z), (1.0, 0.0, 0.0), near, 1.25)
    for p in (0, 1, 3):
        c.ray((-1.0, _centre(p, H), _centre(7 - p, H)), (1.0, 0.0, 0.0), 9 / 2048, 0.9375, noise=0.5)
    return c                                          # N = 15


def _case_coarse():
    """max_steps = 16: dt_min = 0.2165, about one lattice point per level-0 cell — single-sample runs.  N = 16."""
    H = 8
    pats = ("#.#.#.#.", "########", ".#.#.#.#", "#..#..#.")
    entries = []
    for p, pat in enumerate(pats):
        entries += row(0, 1, p + 1, p + 2, pat)
    c = Case("coarse16", Grid(H, 1, 1.0, entries), 16)
    for p in range(len(pats)):
        for near, ns in ((1 / 32, 0.0), (3 / 32, 0.0), (1 / 32, 0.5), (5 / 64, 0.0)):
            c.ray((_centre(p + 1, H), -1.0, _centre(p + 2, H)), (-0.0, 1.0, 0.0), near, 2.5, noise=ns)
    return c


def _case_tiny(max_steps, N):
    """max_steps 1 and 4: dt_min > dt_max, clampf returns dt_max; a cap of one sample."""
    H = 8
    entries = row(0, 2, 3, 4, "########") + row(0, 2, 4, 3, ".#.##.##")
    c = Case(f"tiny{max_steps}", Grid(H, 1, 1.0, entries), max_steps)
    for n in range(N):
        full = n % 2 == 0
        c.ray((_centre(3 if full else 4, H), _centre(4 if full else 3, H), -1.0), (0.0, 0.0, 1.0), (1 + 2 * n) / 64, 1.9375)
    return c


def _first_near(pred, q=1024, lo=1, hi=400):
    for k in range(lo, hi):
        if pred(k / q):
            return k / q
    raise AssertionError("no phase found")


def _case_cap():
    """The max_steps cap with samples already out, in the middle of a chunk, on a chunk boundary, at the last point of a run,
    and walks that end by themselves with max_steps and max_steps - 1 samples.  Rays of direction (1/2, 0, 0) and
    (1/4, 0, 0) put 148 and 296 lattice points into a cell, so a row inside the box holds more than max_steps.  N = 33."""
    H = 8
    pats = ("########", ".#######", "#######.", "#.###...", "#.#####.")
    entries = []
    for p, pat in enumerate(pats):
        entries += row(0, 0, p, p + 2, pat)
    c = Case("cap", Grid(H, 1, 1.0, entries), 1024)
    yz = lambda p: (_centre(p, H), _centre(p + 2, H))

    def emitted(near, speed, pat, far=1e9):
        ts = _axis_lattice(near, 1024, 2600).astype(np.float64)
        ts = ts[ts < far]
        cells = np.minimum(np.floor(ts * speed * 4).astype(int), 7)
        return np.nonzero(np.array([ch == "#" for ch in pat])[cells])[0], ts

    for p in (0, 1):                                   # the cap inside a run: on the boundary 16 * 64, and at lane ~10 of chunk 17
        for near in (3 / 1024, 40 / 1024, 77 / 1024):
            c.ray((-1.0,) + yz(p), (0.5, 0.0, 0.0), near, 3.96875 if near != 40 / 1024 else 0.71875, tag="cap_in_run")
    c.ray((-1.0,) + yz(0), (1.0, 0.0, 0.0), 3 / 1024, 3.9375, tag="cap_in_run_clamped")   # behind the box the cell stays H - 1

    def ends_with_run(speed, pat, boundary):
        def pred(near):
            em, ts = emitted(near, speed, pat, 7.9 if speed == 0.25 else 3.96875)
            if len(em) < 1024:
                return False
            e = int(em[1023])
            nxt_empty = e + 1 < len(ts) and (len(em) == 1024 or em[1024] != e + 1)
            return nxt_empty and ((e + 1) % 64 == 0) == boundary
        return pred
    n1 = _first_near(ends_with_run(0.5, pats[2], True))            # "#######.": samples 0 .. 1023, the empty lane is lane 0
    c.ray((-1.0,) + yz(2), (0.5, 0.0, 0.0), n1, 3.96875, tag="cap_run_end_boundary")
    n2 = _first_near(ends_with_run(0.25, pats[3], False), lo=400, hi=1024)   # the 1024th sample ends its run, mid-chunk
    c.ray((-1.0,) + yz(3), (0.25, 0.0, 0.0), n2, 7.9, tag="cap_run_end")
    # walks that end by themselves: far = the float above / exactly the lattice point of sample 1024
    near = 5 / 1024
    ts = _axis_lattice(near, 1024, 1100)
    c.ray((-1.0,) + yz(0), (0.5, 0.0, 0.0), near, float(np.nextafter(ts[1023], F(9))), tag="natural_max")
    c.ray((-1.0,) + yz(0), (0.5, 0.0, 0.0), near, float(ts[1023]), tag="natural_max_minus_1")
    c.ray((-1.0,) + yz(2), (0.5, 0.0, 0.0), n1, 3.6, tag="natural_max")
    k = 0
    while c.N < 33:                                    # the other patterns from other phases
        p = k % len(pats)
        c.ray((-1.0,) + yz(p), (0.5 if k % 3 else 0.25, 0.0, 0.0), (11 + 17 * k) / 1024, 0.59375 if k % 3 else 1.21875,
              noise=0.5 if k % 4 == 1 else 0.0)
        k += 1
    return c


def _case_c2():
    """C = 2, bound 2, H = 8.  The full grid: an axis ray holds ~1180 lattice points and stops at 16 * 64.  A checkered
    grid: rays of all eight octants with small-integer directions.  N = 17 + 16."""
    H = 8
    full = [(l, (x, y, z)) for l in range(2) for x in range(H) for y in range(H) for z in range(H)]
    c = Case("c2_full", Grid(H, 2, 2.0, full), 1024)
    for k in range(17):
        a, s = k % 3, 1.0 if k % 2 else -1.0
        o = [0.125 + 0.25 * (k % 5), -0.625 + 0.25 * (k % 4)]
        o.insert(a, -2.0 * s)
        d = [0.0, -0.0]
        d.insert(a, s)
        c.ray(o, d, (3 + 5 * k) / 1024, 3.984375 if k < 2 else 0.703125, noise=0.5 if k % 5 == 4 else 0.0)
    check = [(l, (x, y, z)) for l in range(2) for x in range(H) for y in range(H) for z in range(H)
             if (x + 2 * y + 3 * z + l) % 4 in (0, 1)]
    e = Case("c2_octants", Grid(H, 2, 2.0, check), 1024)
    for k in range(16):
        sx, sy, sz = (1 if k & 1 else -1), (1 if k & 2 else -1), (1 if k & 4 else -1)
        d = (sx * 1.0, sy * 0.5, sz * 0.25) if k < 8 else (sx * 1.0, sy * 2.0, sz * 3.0)
        o = (-sx * 1.90625, -sy * (0.8125 if k < 8 else 1.96875), -sz * (0.34375 if k < 8 else 1.9375))
        e.ray(o, d, 7 / 1024, 2.75 if k < 8 else 1.28125)
    return c, e


def _case_straddle():
    """bound 1.5 at C = 2: mip_bound = min(2, 1.5), level-1 cells of 0.375 whose faces are not the unit cube's.  The level-1
    cell [0.75, 1.125] holds points of level 0: a ray that meets it EMPTY from outside jumps over the occupied level-0 cell
    [0.75, 1) — the one place where a jump differs from walking point by point, which gives the pending-exit mistakes and
    the sign-of-zero mistakes something to change."""
    H = 8
    tr = (0.125, -0.625)                              # transverse coordinates: level-0 cells 4, 1; level-1 cells 4, 2
    l0 = lambda v: math.floor((v + 1) / 2 * H)
    l1 = lambda v: math.floor((v / 1.5 + 1) / 2 * H)
    entries = []
    for axis in range(3):
        entries += row(0, axis, l0(tr[0]), l0(tr[1]), "#.#..#.#")       # level 0: the outer cells [-1, -0.75), [0.75, 1) occupied
        entries += row(1, axis, l1(tr[0]), l1(tr[1]), "#......#")       # level 1: only the outermost cells
    c = Case("straddle", Grid(H, 2, 1.5, entries), 1024)
    for axis in range(3):
        for s in (1.0, -1.0):
            for z0, z1 in AXIS_ZEROS:
                for near in (9 / 1024, 30 / 1024, 51 / 1024):
                    o = list(tr)
                    o.insert(axis, -s * 1.46875)
                    d = [z0, z1]
                    d.insert(axis, s)
                    c.ray(o, d, near, 2.9375 if (near == 9 / 1024 and (z0, z1) == (0.0, 0.0) and s > 0) else 0.78125)
    return c


def _case_levels3():
    """C = 3, bound 4, H = 16: an axis ray crosses levels 2 -> 1 -> 0 -> 1 -> 2.  max_steps 1024 gives 2300 lattice points."""
    H = 16
    tr = (0.0625, -0.1875)
    cells = lambda lvl: (math.floor((tr[0] / 2 ** lvl + 1) / 2 * H), math.floor((tr[1] / 2 ** lvl + 1) / 2 * H))
    entries = []
    for axis in range(3):
        entries += row(0, axis, *cells(0), "#..#....#.#..#.#")
        entries += row(1, axis, *cells(1), "#.#.#..##..#.#.#")
        entries += row(2, axis, *cells(2), ".#.#.#.##.#.#.#.")
    c = Case("levels3", Grid(H, 3, 4.0, entries), 1024)
    for k in range(15):
        axis, s = k % 3, 1.0 if k % 2 else -1.0
        o = list(tr)
        o.insert(axis, -s * 3.96875)
        d = [0.0, 0.0] if k < 8 else [-0.0, 0.0]
        d.insert(axis, s)
        c.ray(o, d, (5 + 14 * k) / 1024, 7.90625 if k < 3 else 4.53125 if k < 6 else 1.53125, noise=0.5 if k == 14 else 0.0)
    return c                                          # N = 15


def _case_gamma():
    """dt_gamma = 1/16 at C = 2, bound 2, H = 16: dt = t / 16 between dt_min and dt_max, and from t = 2 on the level of
    dt * H / 2 = t / 2 is 1 — inside the unit cube, where the position alone says level 0."""
    H = 16
    tr = (0.0625, -0.3125)
    cells = lambda lvl: (math.floor((tr[0] / 2 ** lvl + 1) / 2 * H), math.floor((tr[1] / 2 ** lvl + 1) / 2 * H))
    entries = []
    for axis in range(3):
        entries += row(0, axis, *cells(0), "##.#.##.#..###.#")
        entries += row(1, axis, *cells(1), ".#.#####...#.#.#")
    c = Case("gamma", Grid(H, 2, 2.0, entries), 1024, dt_gamma=1 / 16)
    for k in range(17):
        axis, s = k % 3, 1.0 if k % 2 else -1.0
        o = list(tr)
        o.insert(axis, -s * 1.96875)
        d = [0.0, -0.0]
        d.insert(axis, s * 0.5)
        c.ray(o, d, (40 + 37 * k) / 1024, 7.8125, noise=(0.0, 0.5)[k % 2])
    return c                                          # N = 17


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        c2, c2o = _case_c2()
        lst = [_case_rows8(), _case_axes(), _case_rows2048(), _case_coarse(), _case_tiny(1, 1), _case_tiny(4, 15),
               _case_cap(), c2, c2o, _case_straddle(), _case_levels3(), _case_gamma()]
        _CASES = {c.name: c for c in lst}
    return _CASES


def case_names():
    return list(cases())


def lidar_case(name):
    """The case with noise 0 (the alive-ray marcher takes no perturbation)."""
    c = cases()[name]
    if "lidar" not in c._derived:
        c._derived["lidar"] = c.derived(name + "/noise0", noise=[0.0] * c.N)
    return c._derived["lidar"]


def serial_case(name, n_step, noise):
    """Single calls of the serial template: every ray starts at a lattice point of its own walk (the point of the
    sample two thirds along, or t_0), perturbed by `noise`, and takes at most n_step samples (the template has no max_steps cap)."""
    c = lidar_case(name)
    key = ("serial", n_step, noise)
    if key not in c._derived:
        walks = march_model(c)
        combo = 2 * N_STEPS_SERIAL.index(n_step) + (1 if noise else 0)      # 0 .. 5, one per (n_step, noise) pair
        keep = [n for n in range(c.N) if (n + combo) % 6 == 0 or c.N < 6]   # every ray starts one of the six kinds of call
        near = {}
        for n in keep:
            w = walks[n]
            i = w.idx[(2 * len(w.idx)) // 3] if w.idx and n % 2 else 0
            near[n] = float(case_ray(c, n).lat.T(i))
        c._derived[key] = c.derived(f"{name}/serial{n_step}/{noise}", near=near, noise={n: noise for n in keep}, max_cap=n_step,
                                    keep=keep)
    return c._derived[key]


# ================================================================================================ coverage
PROMISED = (
    "empty: exit in chunk c + 1", "empty: exit in chunk c + 2 (a whole chunk skipped)", "empty: exit in chunk >= c + 3",
    "empty: exit on lane 0", "empty: exit on lane 63", "empty: two in a row, the second exit pending", "empty: first lattice point",
    "run: crosses one chunk boundary", "run: crosses two chunk boundaries", "run: fills a chunk (run >= 64)",
    "run: ends on lane 63", "run: starts on lane 0 right behind a pending exit", "run: a single sample",
    "cap: max_steps = 1", "cap: in chunk >= 1 inside a run", "cap: at the last point of a run",
    "cap: at the decision for an empty lane", "cap: exactly at a chunk boundary",
    "cap: exactly at a chunk boundary, C = 2 bound 2 full grid", "cap: the walk ends by itself with count = max_steps",
    "cap: the walk ends by itself with count = max_steps - 1", "cap: dt_min > dt_max",
    "far: inside a run, mid-chunk", "far: on lane 0", "far: inside a pending empty cell", "far: equal to a lattice point",
    "far: the float below a lattice point", "far: the float above a lattice point", "far: far < near", "far: NaN",
    "direction: all eight octants", "direction: plane-parallel", "direction: |d| != 1",
    "level: 2 -> 1 -> 0 -> 1 -> 2 at C = 3", "level: bound 1.5 at C = 2", "level: raised by dt_gamma inside the unit cube",
    "level: a position clamped at the bound, cell H - 1",
    "noise: 0", "noise: 0.5", "noise: the float below 1",
    "N = 1", "N = 15", "N = 16", "N = 17", "N = 33",
) + tuple(f"direction: axis {a}{s} with zeros {z}" for a in "xyz" for s in "+-" for z in ("+0", "-0"))


def coverage():
    """What the case list reaches, from the model's bookkeeping of lattice index // 64 and % 64: {item: number of rays}.
    Every PROMISED item is in the table, at 0 where nothing reaches it; items beyond the promise are extras."""
    cov = {k: 0 for k in PROMISED}

    def hit(k, cond=True):
        cov[k] = cov.get(k, 0) + (1 if cond else 0)

    octants, axes = set(), set()
    for c in cases().values():
        walks = march_model(c)
        o, d, near, far, noise = c.arrays()
        hit(f"N = {c.N}")
        for n, w in enumerate(walks):
            ray = case_ray(c, n)
            ch = lambda i: i // 64
            em = set(w.idx)
            for k, (i, j) in enumerate(w.empties):
                inside = j < ray.n_valid
                hit("empty: exit in chunk c + 1", inside and ch(j) == ch(i) + 1)
                hit("empty: exit in chunk c + 2 (a whole chunk skipped)", inside and ch(j) == ch(i) + 2)
                hit("empty: exit in chunk >= c + 3", inside and ch(j) >= ch(i) + 3)
                hit("empty: exit on lane 0", inside and j % 64 == 0)
                hit("empty: exit on lane 63", inside and j % 64 == 63)
                hit("empty: first lattice point", i == 0)
                if k + 1 < len(w.empties):
                    i2, j2 = w.empties[k + 1]
                    hit("empty: two in a row, the second exit pending", i2 == j and ch(j2) > ch(i2))
                hit("far: inside a pending empty cell", not inside and ch(ray.n_valid) > ch(i))
                hit("far: inside an empty cell, same chunk", not inside and ch(ray.n_valid) == ch(i))
                hit("run: starts on lane 0 right behind a pending exit", inside and j % 64 == 0 and ch(i) < ch(j) and j in em)
            runs, capped = [], w.end == "cap"
            for i in w.idx:
                if runs and runs[-1][1] == i - 1:
                    runs[-1][1] = i
                else:
                    runs.append([i, i])
            for k, (a, b) in enumerate(runs):
                cut = capped and k == len(runs) - 1
                hit("run: crosses one chunk boundary", ch(b) == ch(a) + 1)
                hit("run: crosses two chunk boundaries", ch(b) >= ch(a) + 2)
                hit("run: fills a chunk (run >= 64)", ch(b) - ch(a) >= 2 or (a % 64 == 0 and b - a >= 63))
                hit("run: ends on lane 63", b % 64 == 63 and not cut and b + 1 < ray.n_valid)
                hit("run: a single sample", a == b and not cut and b + 1 < ray.n_valid)
            if capped:
                e = w.idx[-1]
                nxt_valid = e + 1 < ray.n_valid
                nxt_occ = nxt_valid and ray.geo(e + 1).occ
                hit("cap: max_steps = 1", c.max_steps == 1)
                hit("cap: in chunk >= 1 inside a run", ch(e) >= 1 and nxt_occ and (e + 1) % 64 != 0 and w.idx[0] > 0)
                hit("cap: at the last point of a run", nxt_valid and not nxt_occ)
                hit("cap: at the decision for an empty lane", nxt_valid and not nxt_occ and (e + 1) % 64 != 0)
                hit("cap: exactly at a chunk boundary", nxt_valid and (e + 1) % 64 == 0)
                hit("cap: exactly at a chunk boundary, C = 2 bound 2 full grid", nxt_occ and (e + 1) == 16 * 64 and c.grid.C == 2)
            hit("cap: the walk ends by itself with count = max_steps", w.end == "far" and len(w.idx) == c.max_steps)
            hit("cap: the walk ends by itself with count = max_steps - 1", w.end == "far" and len(w.idx) == c.max_steps - 1)
            hit("cap: dt_min > dt_max", ray.lat.dt_min > ray.lat.dt_max and len(w.idx) > 0)
            if w.end == "far" and w.idx and w.idx[-1] == ray.n_valid - 1:
                hit("far: inside a run, mid-chunk", ray.n_valid % 64 != 0 and ray.geo(ray.n_valid).occ)
                hit("far: on lane 0", ray.n_valid % 64 == 0)
            tag = c.tags[n]
            nv = ray.n_valid
            if tag == "far_eq":
                hit("far: equal to a lattice point", _bits(ray.lat.T(nv)) == _bits(far[n]) and nv - 1 in em)
            if tag == "far_below":
                hit("far: the float below a lattice point", _bits(np.nextafter(far[n], F(9))) == _bits(ray.lat.T(nv)) and nv - 1 in em)
            if tag == "far_above":
                hit("far: the float above a lattice point", _bits(np.nextafter(far[n], F(0))) == _bits(ray.lat.T(nv - 1)) and nv - 1 in em)
            hit("far: far < near", far[n] < near[n] and nv == 0)
            hit("far: NaN", bool(np.isnan(far[n])) and len(w.idx) == 0)
            nz = [bool(v != 0) for v in d[n]]
            if all(nz) and w.idx:
                octants.add(tuple(bool(v > 0) for v in d[n]))
            if sum(nz) == 1 and w.idx:
                a = nz.index(True)
                axes.add((a, bool(d[n][a] > 0), tuple(bool(np.signbit(d[n][b])) for b in range(3) if b != a)))
            hit("direction: plane-parallel", sum(nz) == 2 and len(w.idx) > 0)
            hit("direction: |d| != 1", abs(sum(float(v) ** 2 for v in d[n]) - 1) > 0.1 and len(w.idx) > 0)
            lv = [k for k, _ in _groups(w.levels)]
            hit("level: 2 -> 1 -> 0 -> 1 -> 2 at C = 3", c.grid.C == 3 and _has_subsequence(lv, [2, 1, 0, 1, 2]))
            hit("level: bound 1.5 at C = 2", c.grid.bound == 1.5 and c.grid.C == 2 and 1 in lv and 0 in lv)
            vis = [ray.geo(i) for i in w.visited]
            hit("level: raised by dt_gamma inside the unit cube", any(g.level_dt > g.level_pos for g in vis))
            hit("level: a position clamped at the bound, cell H - 1",
                any(any(cl and ce == c.grid.H - 1 for cl, ce in zip(g.clamped, g.cell)) for g in vis))
            hit("noise: 0", noise[n] == 0)
            hit("noise: 0.5", noise[n] == 0.5)
            hit("noise: the float below 1", _bits(noise[n]) == _bits(np.nextafter(F(1), F(0))))
    cov["direction: all eight octants"] = len(octants) // 8
    for a in range(3):
        for pos in (True, False):
            for zs in ((False, False), (True, True)):
                k = f"direction: axis {'xyz'[a]}{'+' if pos else '-'} with zeros {'-0' if zs[0] else '+0'}"
                cov[k] = int((a, pos, zs) in axes)
    return cov


def _groups(seq):
    out = []
    for v in seq:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return out


def _has_subsequence(seq, want):
    k = 0
    for v in seq:
        if k < len(want) and v == want[k]:
            k += 1
    return k == len(want)


# ================================================================================================ the old profile
def old_profile_points_per_empty_cell(n_rays=12, cascade=2):
    """The family tests/test_raymarch_gpu.py and its siblings march: H = 128, max_steps = 1024, C <= 2, a sphere of random cells,
    rays from one bundle behind the -x face.  Returns the largest number of lattice points the model skips in one empty cell
    (exit index - met index): below 64, no chunk ever lies inside an empty cell."""
    H = 128
    rng = np.random.default_rng(3)
    entries = []
    for lvl in range(cascade):
        for _ in range(3000):
            x, y, z = (int(v) for v in rng.integers(0, H, 3))
            if (x - 64) ** 2 + (y - 64) ** 2 + (z - 64) ** 2 < (0.3 * H) ** 2:
                entries.append((lvl, (x, y, z)))
    g = Grid(H, cascade, float(cascade), entries, committed_size=False)
    c = Case("old_profile", g, 1024, 0.0 if cascade == 1 else 1 / 128)
    for k in range(n_rays):
        o = (-0.8 * g.bound + (rng.integers(-8, 8) / 128), 0.1 + rng.integers(-8, 8) / 128, rng.integers(-8, 8) / 128)
        d = (1.0, rng.integers(-40, 40) / 64, rng.integers(-40, 40) / 64)
        c.ray(o, d, 0.0625, 1.5 * g.bound)
    worst = 0
    for w in march_model(c):
        for i, j in w.empties:
            worst = max(worst, j - i)
    bound = max(2 ** lvl * 1024 / H for lvl in range(cascade))   # at most 2^level * max_steps / H lattice points fit a cell
    return worst, bound
