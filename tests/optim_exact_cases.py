"""Problems and references of the exact tests of the optimizer step (csrc/optim.hip): lnh_grad_check_f16, lnh_adam_table_step(_dlr),
lnh_train_check, lnh_train_step, lnh_zero_regions.  NumPy only; tests/test_optim_exact_cpu.py asserts the conditions stated here,
tests/test_optim_exact_gpu.py runs the kernels against them ("Exact tests of the optimizer step").

The references restate the header's text (include/lidarnerf_hip.h, optimizer section) and the arithmetic comment of optim.hip:
  1. adam_scalars / unscale / moments_f32 / param_f32: Adam for one element as the kernels round it (tier A, bit for bit);
  2. adam_f64: plain Adam in float64 with, per element, A = the sum of the absolute addends of the update (tier B);
  3. train_check / train_step: the bookkeeping as a state machine over the 12 used floats of `state`;
  4. bad16 / bad32: the finite predicate on raw bit patterns;
  5. MISTAKES: named wrong variants of 1, 3, 4 and of where the kernels walk (every function takes `mistake=`).
Supposed: float32 division and sqrtf are correctly rounded (hipcc's default); float <-> double and float -> half conversions round to
nearest even; the double pow is used only where its result is exact, or is allowed one neighbour (see candidates()).
Out of scope: exp_avg_sq in the float32 subnormal range (the inputs keep it above 2^-100), a loss scale backed off into the
subnormals, step counts past 2^24 (the counters are floats).
"""
import collections
import functools
import math

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
U = 2.0 ** -24
EPS = 1e-15
WG = 256
TABLE_WG_CAP, CHECK_WG_CAP, SMALL_WG_CAP, ZERO_WG_CAP = 4096, 2048, 64, 1024
MAX_SMALL, STATE_FLOATS = 16, 16
SCALE, GROWTH, FOUND, INV, INV_TABLE, LAST_SCALE, T, IT, LR, T_NEXT, IT_NEXT, SKIPPED = range(12)
SLOT_NAMES = ("SCALE", "GROWTH", "FOUND", "INV", "INV_TABLE", "LAST_SCALE", "T", "IT", "LR", "T_NEXT", "IT_NEXT", "SKIPPED")

TRIP = TABLE_WG_CAP * WG * 4                      # values one trip of the table walk covers: 4 194 304
CHECK_TRIP = CHECK_WG_CAP * WG * 8                # ... and one trip of the finite check: the same number
SMALL_TRIP = SMALL_WG_CAP * WG                    # elements of a small tensor one trip covers: 16 384
N_BIG = 4 * (1048576 + 300) + 3                   # a second trip of 300 vectors and a 3-element tail
N_SMALL_SHAPES = (1, 2, 3, 4, 5, 1023, 1024, 1027)
N_BOUNDARY = (4 * 1048320, 4 * 1048321, 4 * 1048576)   # 4095 + 1 blocks | the cap takes over | the last size of one trip
PROD_BETAS, EXACT_BETAS = (0.9, 0.99), (0.5, 0.75)     # 0.5^t and 0.75^t are exact doubles for every t used here

MISTAKES = (
    # arithmetic: each of these must also break the tier B bound (ARITHMETIC below)
    "bias_t_minus_1", "bc2_no_sqrt", "eps_inside_sqrt", "v_uses_beta1", "grad_not_unscaled",
    # roundings only: tier A alone can see them
    "m_float32_axpy", "p16_from_old_p",
    # where the kernels walk
    "tail_off_by_one", "second_trip_stride_griddim", "small_moment_offset_null",
    # finite check
    "check_mask_drops_halfword",
    # bookkeeping
    "stamp_ge", "stamp_nonzero", "growth_no_isfinite", "inv_uses_div_table", "schedule_clamp_dropped",
)
ARITHMETIC = MISTAKES[:5]
# Not in the list: "the head length of k_zero_regions in bytes instead of words".  It changes no output — head + 4 * n4 + rest is
# still every word of the region, only the 16-byte stores lose their alignment — so no known-answer test can see it.


def block_count(n, per_thread, cap):
    """Workgroups of a grid-stride launch over n values, `per_thread` values a thread (the host formula, restated)."""
    nv = n // per_thread
    full = (nv + WG - 1) // WG
    return full + 1 if full < cap else cap


# ================================================================================================ 1. Adam as the kernels round it
def adam_scalars(lr, b1, b2, t, mistake=None):
    """(step_size, bc2_sqrt) as float32.  `lr` is the double the kernel divides: the argument, or the float32 state value."""
    tt = t - 1 if mistake == "bias_t_minus_1" else t
    with np.errstate(all="ignore"):
        bc1, bc2 = F64(1.0) - F64(b1) ** tt, F64(1.0) - F64(b2) ** tt
        return F32(F64(lr) / bc1), F32(bc2 if mistake == "bc2_no_sqrt" else np.sqrt(bc2))


def candidates(lr, b1, b2, t):
    """The nine (step_size, bc2_sqrt) pairs a double pow that is off by an ulp or so can lead to: each scalar is the reference
    float32 or one of its two neighbours.  Labels are (d_step, d_bc2) in {-1, 0, 1}."""
    s, b = adam_scalars(lr, b1, b2, t)
    nb = lambda x, d: x if d == 0 else np.nextafter(x, F32(d * np.inf), dtype=F32)
    order = sorted(((ds, db) for ds in (0, -1, 1) for db in (0, -1, 1)), key=lambda c: abs(c[0]) + abs(c[1]))
    return [((ds, db), nb(s, ds), nb(b, db)) for ds, db in order]


def unscale(gbits, inv, mistake=None):
    """fp16 bit patterns -> g = fl32(fl32(g16) * inv)."""
    g = np.ascontiguousarray(gbits, dtype=np.uint16).view(F16).astype(F32)
    return g if mistake == "grad_not_unscaled" else g * F32(inv)


def moments_f32(m, v, g, b1, b2, mistake=None):
    """m = fl32(m + w1 (g - m)), v = fl32(b2 v + (w2 g) g): float64 operations, each rounded, then one rounding to float32."""
    w1 = 1.0 - b1
    gd, md, vd = g.astype(F64), m.astype(F64), v.astype(F64)
    if mistake == "m_float32_axpy":
        m1 = F32(b1) * m + F32(w1) * g
    else:
        m1 = (md + w1 * (gd - md)).astype(F32)
    bb = b1 if mistake == "v_uses_beta1" else b2
    v1 = (bb * vd + ((1.0 - bb) * gd) * gd).astype(F32)
    return m1, v1


def param_f32(p, m1, v1, step_size, bc2_sqrt, mistake=None):
    """p = fl32(p - fl32(fl32(step_size m) / fl32(fl32(fl32(sqrt v) / bc2_sqrt) + eps))) in float32; p16 = fl16(p)."""
    eps = F32(EPS)
    with np.errstate(all="ignore"):
        if mistake == "eps_inside_sqrt":
            den = np.sqrt(v1 + eps) / F32(bc2_sqrt)
        else:
            den = np.sqrt(v1) / F32(bc2_sqrt) + eps
        p1 = p - (F32(step_size) * m1) / den
        p16 = (p if mistake == "p16_from_old_p" else p1).astype(F16)
    assert p1.dtype == F32 and den.dtype == F32
    return p1, p16


def adam_f32(p, m, v, gbits, inv, lr, b1, b2, t, mistake=None, scalars=None):
    """One step: (p, m, v, p16).  `scalars`: a (step_size, bc2_sqrt) pair in place of adam_scalars()."""
    m1, v1 = moments_f32(m, v, unscale(gbits, inv, mistake), b1, b2, mistake)
    s, b = scalars if scalars is not None else adam_scalars(lr, b1, b2, t, mistake)
    p1, p16 = param_f32(p, m1, v1, s, b, mistake)
    return p1, m1, v1, p16


def adam_f32_values(p, m, v, g, inv, lr, b1, b2, t, mistake=None, scalars=None):
    """The same for a small tensor, whose gradient is float32: g = fl32(g * inv)."""
    gs = g if mistake == "grad_not_unscaled" else g * F32(inv)
    m1, v1 = moments_f32(m, v, gs, b1, b2, mistake)
    p1, _ = param_f32(p, m1, v1, *(scalars if scalars is not None else adam_scalars(lr, b1, b2, t, mistake)), mistake)
    return p1, m1, v1


def walk_table(n, before, after, entry, small_blocks=0, mistake=None):
    """Which elements a step reaches: all of them.  The two walk mistakes leave some as they were."""
    out = [a.copy() for a in after]
    stay = np.zeros(n, dtype=bool)
    if mistake == "tail_off_by_one" and n % 4:
        stay[n - 1] = True
    if (mistake == "second_trip_stride_griddim" and entry == "train_step" and small_blocks
            and block_count(n, 4, TABLE_WG_CAP) == TABLE_WG_CAP):
        lo, hi = TRIP, min(TRIP + small_blocks * WG * 4, (n // 4) * 4)   # vectors the longer stride jumps over
        stay[lo:hi] = True
    for o, b in zip(out, before):
        o[stay] = b[stay]
    return out


# ================================================================================================ 2. Adam in float64
Adam64 = collections.namedtuple("Adam64", "p m v am A")


def adam_f64(st, gbits, inv, lr, b1, b2, t):
    """Plain Adam in float64 on the state `st` (Adam64; am = sum of the absolute addends of m).  A = |p| + the update with every
    addend of m taken by its absolute value: what one rounding of the float32 chain is measured against."""
    g = np.ascontiguousarray(gbits, dtype=np.uint16).view(F16).astype(F64) * F64(inv)
    m = b1 * st.m + (1.0 - b1) * g
    v = b2 * st.v + (1.0 - b2) * g * g
    am = b1 * st.am + (1.0 - b1) * np.abs(g)
    den = np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + EPS
    step = F64(lr) / (1.0 - b1 ** t)
    A = np.abs(st.p) + step * am / den
    return Adam64(st.p - step * m / den, m, v, am, A)


def k_of_step(s):
    """Roundings of the float32 chain at the s-th step from zero moments, in units of 2^-24 A (first order; counted on the text):
      g = g16 * inv                 1        m carries s roundings of its own and 1 of every g:      s + 1   (of A_m)
      v: g * g twice g's, s own     s + 2    sqrtf halves that and rounds; / bc2_sqrt (a rounded constant) 2; + eps 1 + 1:
                                             the denominator                                          s / 2 + 5
      step_size (rounded) * m       2        the division 1, the subtraction from p 1
    K(s) = (s + 1) + 2 + (s / 2 + 5) + 1 + 1 = 1.5 s + 10, and 1 for the second-order terms and the roundings in double."""
    return math.ceil(1.5 * s) + 11


# ================================================================================================ 3. the bookkeeping
def new_state(scale=1024.0, **slots):
    st = np.zeros(STATE_FLOATS, dtype=F32)
    st[SCALE] = scale
    for k, val in slots.items():
        st[SLOT_NAMES.index(k)] = val
    return st


def train_check(st, bad, div_table, div_small, lr0, iters, mistake=None):
    """lnh_train_check on a copy of `st`: commit, 1 / scale, the learning rate, the stamp."""
    st = st.copy()
    it = st[IT_NEXT]
    st[T], st[IT] = st[T_NEXT], it
    with np.errstate(all="ignore"):
        inv = F32(1.0) / st[SCALE]
        st[INV] = inv / F32(div_table if mistake == "inv_uses_div_table" else div_small)
        st[INV_TABLE] = inv / F32(div_table)
    st[LAST_SCALE] = st[SCALE]
    x = float(it) / float(iters)
    st[LR] = F32(F64(lr0) * F64(0.1) ** (x if mistake == "schedule_clamp_dropped" else min(x, 1.0)))
    if bad:
        st[FOUND] = it + F32(1.0)
    return st


def lr_is_exact(it, iters):
    """The power of the schedule is 1 or 0.1 itself: any pow returns it."""
    return it == 0 or it >= iters


def train_step(st, growth=2.0, backoff=0.5, interval=2000, mistake=None):
    """The books of lnh_train_step on a copy of `st`: (state, skipped).  Scale update = torch's amp_update_scale_."""
    st = st.copy()
    stamp = st[IT] + F32(1.0)
    skip = bool(st[FOUND] >= stamp if mistake == "stamp_ge" else st[FOUND] != 0 if mistake == "stamp_nonzero" else st[FOUND] == stamp)
    st[T_NEXT] = st[T] if skip else st[T] + F32(1.0)
    st[IT_NEXT] = stamp
    st[SKIPPED] = 1.0 if skip else 0.0
    with np.errstate(all="ignore"):
        if skip:
            st[SCALE], st[GROWTH] = st[SCALE] * F32(backoff), 0.0
        elif st[GROWTH] + F32(1.0) == F32(interval):
            ns = st[SCALE] * F32(growth)
            if np.isfinite(ns) or mistake == "growth_no_isfinite":
                st[SCALE] = ns
            st[GROWTH] = 0.0
        else:
            st[GROWTH] += F32(1.0)
    return st, skip


def amp_update_scale(scale, tracker, found, growth=2.0, backoff=0.5, interval=2000, mistake=None):
    """(scale, tracker) after one update: the scale rule alone, through train_step."""
    st = new_state(scale, GROWTH=tracker, FOUND=1.0 if found else 0.0)
    st, _ = train_step(st, growth, backoff, interval, mistake)
    return float(st[SCALE]), float(st[GROWTH])


Scenario = collections.namedtuple("Scenario", "name init iters lr0 div_table div_small interval steps")
# a step: (bad, preset) — bad: the gradients hold an inf; preset: FOUND := IT_NEXT + preset before the check (None: left alone)
OK, BAD = (False, None), (True, None)
SCENARIOS = (
    Scenario("schedule", {}, 4.0, 2.0 ** -6, 1.0, 1.0, 2000, (OK,) * 10),               # it = 0 .. 9 = iters + 5
    Scenario("growth_interval_1", {}, 4.0, 2.0 ** -6, 2.0, 4.0, 1, (OK, OK, BAD, OK)),
    Scenario("growth_interval_3", {}, 4.0, 2.0 ** -6, 2.0, 4.0, 3, (OK, OK, OK, OK, OK, BAD, OK, OK, OK)),   # the skip arrives at counter 2
    Scenario("scale_at_the_top", {"SCALE": 2.0 ** 127, "GROWTH": 2.0}, 4.0, 2.0 ** -6, 1.0, 1.0, 3, (OK, OK)),
    Scenario("backoff_from_small", {"SCALE": 2.0 ** -10}, 4.0, 2.0 ** -6, 1.0, 2.0, 2000, (BAD, OK)),
    Scenario("stale_stamp", {}, 100.0, 2.0 ** -6, 3.0, 1.0, 2000, (OK, OK, BAD, OK, OK, OK, OK)),
    Scenario("stamp_of_another_rank", {"IT_NEXT": 5.0, "T_NEXT": 5.0}, 4.0, 2.0 ** -6, 1.0, 1.0, 2000,
             ((False, 0), (False, 2), (False, 1), (False, None), (False, 2))),
)


def run_scenario(sc, mistake=None):
    """[(state after the check, state after the step, skipped)] of every step."""
    st, out = new_state(), []
    for k, val in sc.init.items():
        st[SLOT_NAMES.index(k)] = val
    for bad, preset in sc.steps:
        if preset is not None:
            st = st.copy()
            st[FOUND] = st[IT_NEXT] + F32(preset)
        a = train_check(st, bad, sc.div_table, sc.div_small, sc.lr0, sc.iters, mistake)
        st, skip = train_step(a, interval=sc.interval, mistake=mistake)
        out.append((a, st, skip))
    return out


# ================================================================================================ 4. the finite predicate
def bad16(bits, n=None, mistake=None):
    """Does an fp16 gradient of n values (raw uint16 patterns) hold an inf / nan?  Exponent field all ones."""
    bits = np.asarray(bits, dtype=np.uint16)[:n]
    hit = (bits & 0x7c00) == 0x7c00
    if mistake == "check_mask_drops_halfword":   # the high half of the third word of a whole vector goes unchecked
        idx = np.arange(len(bits))
        hit &= ~((idx % 8 == 5) & (idx < len(bits) // 8 * 8))
    return bool(hit.any())


def bad32(bits):
    return bool(((np.asarray(bits, dtype=np.uint32) & 0x7f800000) == 0x7f800000).any())


BAD_PATTERNS = {"+inf": 0x7c00, "-inf": 0xfc00, "quiet_nan": 0x7e00, "signalling_nan": 0x7c01, "negative_nan": 0xfe01}
BAD_PATTERNS32 = {"+inf": 0x7f800000, "-inf": 0xff800000, "quiet_nan": 0x7fc00000, "signalling_nan": 0x7f800001, "negative_nan": 0xffc00001}
CHECK_BASE = CHECK_TRIP + 8 * 300                 # whole vectors of the checked buffer: a second trip of 300 vectors


def check_positions():
    """(n, index) of every bad-value position of the finite-check test."""
    out = [(CHECK_BASE, i) for i in range(8)]                                   # the first vector
    out += [(CHECK_BASE, CHECK_TRIP - 8 + i) for i in range(8)]                 # the last vector of the first trip
    out += [(CHECK_BASE, CHECK_TRIP + i) for i in range(8)]                     # the first vector of the second trip
    out += [(CHECK_BASE, CHECK_BASE - 8 + i) for i in range(8)]                 # the last whole vector
    out += [(CHECK_BASE + tl, CHECK_BASE + j) for tl in range(1, 8) for j in range(tl)]   # every tail, every position
    return out


def finite_fill16(n, seed=11):
    """Finite fp16 patterns that sit next to the bad ones: +-65504, subnormals, +-0."""
    pool = np.array([0x7bff, 0xfbff, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0000, 0x8000, 0x7800, 0x3c00], dtype=np.uint16)
    return pool[np.random.default_rng(seed).integers(0, len(pool), n)]


def finite_fill32(n, seed=12):
    """+-FLT_MAX, float32 subnormals, +-0."""
    pool = np.array([0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0, 0x80000000, 0x7f000000], dtype=np.uint32)
    return pool[np.random.default_rng(seed).integers(0, len(pool), n)]


# ================================================================================================ inputs
@functools.lru_cache(maxsize=None)
def table_params():
    """N_BIG float32 parameters in +-1e-4 (fp16 subnormals below 6.1e-5); every seventh — where the gradient is zero and the
    parameter stays put — is an odd multiple of 2^-25: a tie between two fp16 values, subnormal and normal ones."""
    rng = np.random.default_rng(1)
    p = ((rng.random(N_BIG) - 0.5) * 2e-4).astype(F32)
    ties = ((rng.integers(0, 1678, N_BIG) + 0.5) * 2.0 ** -24 * rng.choice([-1.0, 1.0], N_BIG)).astype(F32)
    z = zero_mask()
    p[z] = ties[z]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def zero_mask():
    return np.arange(N_BIG) % 7 == 0


SPECIALS = (0x7bff, 0xfbff, 0x0001, 0x8001, 0x03ff, 0x0400)   # +-65504, the smallest and largest subnormal, the smallest normal


@functools.lru_cache(maxsize=8)
def table_grad(step):
    """N_BIG fp16 bit patterns of step `step`: uniform over the finite patterns (so over the exponents, subnormals included),
    a seventh of them +-0, the extremes at the front (indices 1 .. 6) and in the tail of N_BIG."""
    rng = np.random.default_rng(100 + step)
    bits = rng.integers(0, 0x7c00, N_BIG).astype(np.uint16) | (rng.integers(0, 2, N_BIG).astype(np.uint16) << 15)
    z = zero_mask()
    bits[z] = np.where(np.arange(N_BIG) % 2 == 0, 0x0000, 0x8000).astype(np.uint16)[z]
    for k, b in enumerate(SPECIALS):
        bits[1 + k] = b
    bits[N_BIG - 3], bits[N_BIG - 2] = 0x7bff, 0x8001   # (N_BIG - 1 is a multiple of 7: a zero)
    bits.setflags(write=False)
    return bits


LR0, ITERS = 2.0 ** -6, 4.0                        # the schedule of the runs; they start at IT = ITERS, where the power is 0.1 itself
RUN_LR = float(F32(F64(LR0) * F64(0.1)))          # ... so LR is this float at every step (a float32: _dlr reads it from the device)
DIV_SMALL = 4.0
INV_SOURCE = {"2^-10": (1024.0, 1.0), "2^-16": (65536.0, 1.0), "1/3072": (1024.0, 3.0)}   # (loss scale, div_table) behind INVS
INVS = {"2^-10": F32(2.0 ** -10), "2^-16": F32(2.0 ** -16), "1/3072": F32(F32(1.0) / F32(1024.0)) / F32(3.0)}
SMALL_NUMEL = (0, 1, 255, 256, 257, 16384, 16385, 16641, 3, 1024, 7, 4099, 64, 2, 513, 33)
SMALL_NULL = (0, 9, 13)            # tensors without a gradient; tensor 0 is also empty
SMALL_BLOCKS = min((max(SMALL_NUMEL) + WG - 1) // WG, SMALL_WG_CAP)


def small_offsets(numel=SMALL_NUMEL, null=SMALL_NULL, mistake=None):
    """Offset of every tensor's moments in the flat buffers: back to back in the order given, gradient or not."""
    off, out = 0, []
    for k, n in enumerate(numel):
        out.append(off)
        if not (mistake == "small_moment_offset_null" and k in null):
            off += n
    return out


@functools.lru_cache(maxsize=None)
def small_inputs():
    """(params, m0, v0): per tensor; the moments of tensor k start at the known values (k + 1) 2^-12 and (k + 1) 2^-20."""
    rng = np.random.default_rng(2)
    ps = [(rng.standard_normal(n) * 0.1).astype(F32) for n in SMALL_NUMEL]
    ms = [np.full(n, (k + 1) * 2.0 ** -12, dtype=F32) for k, n in enumerate(SMALL_NUMEL)]
    vs = [np.full(n, (k + 1) * 2.0 ** -20, dtype=F32) for k, n in enumerate(SMALL_NUMEL)]
    return ps, ms, vs


@functools.lru_cache(maxsize=8)
def small_grads(step):
    """Float32 gradients that still carry the loss scale 1024; None for SMALL_NULL; a tenth of the elements zero."""
    rng = np.random.default_rng(200 + step)
    out = []
    for k, n in enumerate(SMALL_NUMEL):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n) * 1024.0).astype(F32)
        g[rng.random(n) < 0.1] = 0.0
        out.append(None if k in SMALL_NULL else g)
    return out


def small_step(ps, sm, sv, gs, inv, lr, b1, b2, t, mistake=None, scalars=None):
    """One step of all small tensors on the flat moment buffers sm / sv: (params, sm, sv), new arrays."""
    offs, sm, sv, out = small_offsets(mistake=mistake), sm.copy(), sv.copy(), []
    for p, g, o in zip(ps, gs, offs):
        if g is None:
            out.append(p.copy())
            continue
        sl = slice(o, o + len(p))
        p1, sm[sl], sv[sl] = adam_f32_values(p, sm[sl], sv[sl], g, inv, lr, b1, b2, t, mistake, scalars)
        out.append(p1)
    return out, sm, sv


# ================================================================================================ table runs
Run = collections.namedtuple("Run", "name n off betas inv lr steps")   # steps: True = stepped, False = skipped (a bad gradient)


def _runs():
    out = []
    for i, n in enumerate(N_SMALL_SHAPES):   # first steps with the production betas, every inv; four steps with the exact betas
        inv = list(INVS)[i % 3]
        out.append(Run(f"n{n}_first_{inv}", n, 1, PROD_BETAS, inv, RUN_LR, (True,)))
        out.append(Run(f"n{n}_exact_betas", n, 1, EXACT_BETAS, list(INVS)[(i + 1) % 3], RUN_LR, (True, True, False, True, True)))
    for n, inv in zip(N_BOUNDARY, INVS):
        out.append(Run(f"n{n}_first_{inv}", n, 0, PROD_BETAS, inv, RUN_LR, (True,)))
    out.append(Run("big_three_calls", N_BIG, 0, PROD_BETAS, "1/3072", RUN_LR, (True, False, True)))
    for inv in INVS:                         # six steps from zero moments (t = 2 .. 6: one of nine scalar pairs), tier B
        out.append(Run(f"n16387_six_steps_{inv}", 16387, 1, PROD_BETAS, inv, RUN_LR, (True, True, True, False, True, True, True)))
    return tuple(out)


RUNS = _runs()
RUN_NAMES = tuple(r.name for r in RUNS)
SIX_STEP_RUNS = tuple(r.name for r in RUNS if "six_steps" in r.name)


def get_run(name):
    return RUNS[RUN_NAMES.index(name)]


def run_inputs(run):
    """(p0, [gradient bits of every call]) of a run: a window of the shared N_BIG arrays."""
    sl = slice(run.off, run.off + run.n)
    return table_params()[sl], [table_grad(k)[sl] for k in range(len(run.steps))]


def run_reference(run, entry="adam", small_blocks=0, mistake=None):
    """Expected (p, m, v, p16, t) after every call of a run, with adam_scalars() for every t — exact where the powers are, the
    centre of the nine candidates elsewhere.  p16 starts as None: a skipped first call leaves the caller's sentinel."""
    p0, grads = run_inputs(run)
    p, m, v, p16, t = p0.copy(), np.zeros(run.n, F32), np.zeros(run.n, F32), None, 0
    out = []
    for g, stepped in zip(grads, run.steps):
        if stepped:
            t += 1
            new = adam_f32(p, m, v, g, INVS[run.inv], run.lr, *run.betas, t, mistake)
            old = (p, m, v, new[3] if p16 is None else p16)
            p, m, v, p16 = walk_table(run.n, old, new, entry, small_blocks, mistake)
        out.append((p, m, v, p16, t))
    return out


def run_reference64(run, invs=None):
    """[(Adam64, step number s)] after every stepped call of a run.  invs: 1 / scale of every call where it is not the run's
    (lnh_train_step halves the loss scale after a skipped call)."""
    p0, grads = run_inputs(run)
    z = np.zeros(run.n, F64)
    st, t, out = Adam64(p0.astype(F64), z, z, z, z), 0, []
    for k, (g, stepped) in enumerate(zip(grads, run.steps)):
        if stepped:
            t += 1
            st = adam_f64(st, g, INVS[run.inv] if invs is None else invs[k], run.lr, *run.betas, t)
            out.append((st, t))
    return out


def tier_b_ratio(ps, run, invs=None):
    """ps: the float32 parameters after every stepped call.  Largest |p - p64| / bound over elements and steps, where
    bound(s) = bound(s - 1) + K(s) 2^-24 A(s) (the carried error of the state plus this step's roundings), and the largest
    |p - p64| in units of 2^-24 * (the running sum of A)."""
    bound, asum, worst, mult = 0.0, 0.0, 0.0, 0.0
    for p, (st, s) in zip(ps, run_reference64(run, invs)):
        bound = bound + k_of_step(s) * U * st.A
        asum = asum + st.A
        err = np.abs(p.astype(F64) - st.p)
        if not np.isfinite(err).all():
            return math.inf, math.inf
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        mult = max(mult, float((err / np.maximum(U * asum, 1e-300)).max()))
    return worst, mult


# ================================================================================================ lnh_zero_regions
ZERO_BIG_BYTES = 17 * 2 ** 20 + 4                 # past the 1024-workgroup cap of a region (16 MiB)
# (byte offset from a 16-byte boundary, bytes) of the eight regions of a call; None: a null pointer with 0 bytes.  Offsets
# 0 / 4 / 8 / 12 have heads of 0 / 3 / 2 / 1 words; the lengths are shorter than the head, equal to it or just past it.
ZERO_CALL_1 = ((0, 4), (4, 8), (8, 12), (12, 16), (12, 0), None, (4, 20), (4, ZERO_BIG_BYTES))
ZERO_CALL_2 = ((8, 44), (12, 4), (12, 8), (8, 4), (4, 12), (0, 16), (0, 20), (12, 24))
