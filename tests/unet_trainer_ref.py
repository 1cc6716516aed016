"""Float64 restatement of the training step around the ray-drop U-Net's forward and backward (csrc/unet_train_step.hip):
the loss and its cotangent in closed form, clip_grad_norm_ + torch.optim.RMSprop, with the rounding bounds the GPU tests hold the
kernels to and the problems that have one answer.  Pure NumPy / torch on the CPU; tests/test_unet_trainer_cpu.py holds it to golden
G18 and to the stock optimizer."""
import math

import numpy as np
import torch

import unet_ref as R

U = 2.0 ** -24  # unit roundoff of fp32
DICE_EPS = 1e-6


# ---- loss and cotangent ------------------------------------------------------------------------------------------------------------
def loss_terms(x, t, variant=None):
    """(loss, bce part of the gradient, dice part of the gradient) of raydrop_unet_loss in float64, closed form: with s = sigmoid(x),
    I = sum s t, S = sum (s + t), e = 1e-6: dL/dx_i = (s_i - t_i) / M - s_i (1 - s_i) (2 t_i (S + e) - (2 I + e)) / (S + e)^2, the
    dice part 0 and dice = 1 where S == 0.  x, t: float64 arrays of one shape.  `variant` names a deliberately wrong form (the teeth
    of the tests): "no_eps", "t_not_2t", "no_1_over_M", "no_empty_rule"."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    M = x.size
    e = np.exp(-np.abs(x))
    s = np.where(x >= 0, 1.0, e) / (1.0 + e)
    ds = e / ((1.0 + e) * (1.0 + e))
    eps = 0.0 if variant == "no_eps" else DICE_EPS
    I, S = float(np.sum(s * t)), float(np.sum(s + t))
    den, num = S + eps, 2.0 * I + eps
    empty = S == 0.0 and variant != "no_empty_rule"
    bce = float(np.sum(np.maximum(x, 0) - x * t + np.log1p(e))) / M
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = 1.0 if empty else num / den
        two_t = t if variant == "t_not_2t" else 2.0 * t
        g_dice = np.zeros_like(x) if empty else -ds * (two_t * den - num) / (den * den)
    g_bce = (s - t) * (1.0 if variant == "no_1_over_M" else 1.0 / M)
    return bce + (1.0 - dice), g_bce, g_dice


def loss_and_grad(x, t, loss_scale=1.0, variant=None):
    loss, g_bce, g_dice = loss_terms(x, t, variant)
    return loss, (g_bce + g_dice) * loss_scale


def loss_grad_bound(x, t, loss_scale=1.0):
    """(bound of |loss error|, per-element bound of |dlogits error|) for lnh_unet_loss_grad against loss_and_grad.  The kernel forms
    every element in float64 from float64 sums in a fixed order and rounds once to f32.  In §8's model: each float64 operation and
    the M-term chains are off by 2^-53 of their (all-positive) operands per step, exp / log1p by at most 2 ulp; neither part of an
    element goes through more than 64 such steps beyond the chains, so before the store an element is off by at most
    (M + 64) 2^-53 (1 / M + |dice part|) — the BCE part is bounded by 1 / M, not by |s - t| / M, because s carries its error
    relative to s, not to s - t.  The store adds 2^-24 |element|; an element below the smallest normal f32, 2^-126, may lose all of
    itself (a device may flush subnormals), so 2^-126 is the absolute floor."""
    M = np.asarray(x).size
    loss, g_bce, g_dice = loss_terms(x, t)
    chain = (M + 64) * 2.0 ** -53
    per = loss_scale * (U * np.abs(g_bce + g_dice) + chain * (1.0 / M + np.abs(g_dice))) + 2.0 ** -126
    return U * abs(loss) + chain * (abs(loss) + 2.0), per


def loss_grad_ceiling(x, t, loss_scale=1.0):
    """What the bound may nowhere exceed: 2^-18 (1 / M + |dice part|) per element."""
    M = np.asarray(x).size
    return loss_scale * 2.0 ** -18 * (1.0 / M + np.abs(loss_terms(x, t)[2]))


def hashed_loss_case(index, M, keep=0.6):
    """(logits f64 [M] in +-4, masks f64 [M] of 0 / 1), hashed."""
    return 8 * R.hash_u01(9700 + index, M) - 4, (R.hash_u01(9750 + index, M) < keep).astype(np.float64)


# ---- clip + RMSprop ----------------------------------------------------------------------------------------------------------------
def clip_rmsprop(params, grads, square_avgs, bufs, lr, alpha, eps, weight_decay, momentum, max_norm, loss_scale=1.0):
    """One step of clip_grad_norm_(max_norm) on grads / loss_scale + torch.optim.RMSprop in the dtype of the tensors given
    (float64 for the restatement), out of place: (params, square_avgs, bufs, total norm, clip coefficient).  Order:
    total = sqrt(sum g^2) / loss_scale; coef = min(1, max_norm / (total + 1e-6)); g = grad (1 / loss_scale) coef; g += wd p;
    sq = alpha sq + (1 - alpha) g g; avg = sqrt(sq) + eps; buf = momentum buf + g / avg; p -= lr buf."""
    sumsq = sum(float((g.double() ** 2).sum()) for g in grads)
    total = math.sqrt(sumsq) / loss_scale
    coef = min(1.0, max_norm / (total + 1e-6))
    out_p, out_s, out_b = [], [], []
    for p, g, sq, buf in zip(params, grads, square_avgs, bufs):
        g = g * (1.0 / loss_scale) * coef
        if weight_decay != 0:
            g = g + weight_decay * p
        sq = alpha * sq + (1 - alpha) * g * g
        avg = sq.sqrt() + eps
        if momentum > 0:
            buf = momentum * buf + g / avg
            p = p - lr * buf
        else:
            p = p - lr * (g / avg)
        out_p.append(p), out_s.append(sq), out_b.append(buf)
    return out_p, out_s, out_b, total, coef


def rmsprop_bound(p, g_scaled, sq, buf, lr, alpha, eps, weight_decay, momentum, coef, loss_scale):
    """Per-element bounds (|d square_avg|, |d momentum_buffer|, |d param|) of lnh_unet_rmsprop_step against clip_rmsprop in float64
    from the same f32 inputs, with u = 2^-24 per fp32 rounding — each operation of the kernel is rounded on its own, and every
    hyperparameter (1 / loss_scale, coef, wd, alpha, 1 - alpha, eps, momentum, lr) is rounded to f32 once:
      g1 = grad inv coef                 |dg1| <= 4 u |g1|            (inv, coef, two products)
      g  = g1 + wd p                     |dg|  <= |dg1| + 2 u |wd p| + u |g|
      sq' = alpha sq + ((1-alpha) g) g   |dsq'| <= 2 u alpha sq + (1-alpha)(3 u g^2 + 2 |g| |dg|) + u sq'
      avg = sqrt(sq') + eps              |davg| <= |dsq'| / (2 sqrt(sq')) + 2 u sqrt(sq') + u eps + u avg     (sqrtf within 1 ulp)
      q = g / avg                        |dq|  <= |dg| / avg + |q| |davg| / avg + 2 u |q|                      (division within 1 ulp)
      buf' = momentum buf + q            |dbuf'| <= 2 u |momentum buf| + |dq| + u |buf'|
      p' = p - lr buf'                   |dp'| <= lr (2 u |buf'| + |dbuf'|) + u |p'|
    First-order terms, so the whole is multiplied by 1 + 2^-10; where sq' = 0 the square-root term is taken as sqrt(|dsq'|)."""
    p, g_scaled, sq, buf = (t.double() for t in (p, g_scaled, sq, buf))
    g1 = g_scaled / loss_scale * coef
    dg1 = 4 * U * g1.abs()
    g = g1 + weight_decay * p
    dg = dg1 + 2 * U * (weight_decay * p).abs() + U * g.abs()
    sq1 = alpha * sq + (1 - alpha) * g * g
    dsq = 2 * U * alpha * sq + (1 - alpha) * (3 * U * g * g + 2 * g.abs() * dg) + U * sq1
    root = sq1.sqrt()
    droot = torch.where(root > 0, dsq / (2 * root).clamp_min(1e-300), dsq.sqrt())
    avg = root + eps
    davg = droot + 2 * U * root + U * eps + U * avg
    q = g / avg
    dq = dg / avg + q.abs() * davg / avg + 2 * U * q.abs()
    if momentum > 0:
        buf1 = momentum * buf + q
        dbuf = 2 * U * (momentum * buf).abs() + dq + U * buf1.abs()
    else:
        buf1, dbuf = q, dq
    p1 = p - lr * buf1
    dp = lr * (2 * U * buf1.abs() + dbuf) + U * p1.abs()
    k = 1 + 2.0 ** -10
    return dsq * k, dbuf * k, dp * k


# ---- the problem with one answer -----------------------------------------------------------------------------------------------------
EXACT = dict(alpha=0.75, eps=0.0, momentum=0.5, lr=2.0 ** -3, weight_decay=0.0)


def exact_problem(shapes, first_index=9900):
    """(params, [grads of step 1, 2, 3]) f32 for the shapes given: step 1 has gradients +-2^k, k in -3 .. 3, steps 2 and 3
    +-|g1| / 2 with hashed signs, parameters are multiples of 1/4 in +-2.  With EXACT's settings square_avg = g1^2 / 4 after every
    step (0.75 g1^2 / 4 + 0.25 g1^2 / 4), avg = |g1| / 2, g / avg = +-2 then +-1, so momentum_buffer and the parameters stay dyadic
    with a handful of bits: every fp32 operation is exact and any correct implementation gives the same bits."""
    params, steps = [], [[], [], []]
    for i, shape in enumerate(shapes):
        n = int(np.prod(shape))
        u = R.hash_u01(first_index + 4 * i, n)
        params.append(torch.from_numpy(np.floor(u * 17 - 8) / 4).float().reshape(shape))
        k = np.floor(R.hash_u01(first_index + 4 * i + 1, n) * 7).clip(0, 6) - 3
        mag = 2.0 ** k
        for j in range(3):
            sign = np.where(R.hash_u01(first_index + 4 * i + 2, n + j)[j:] < 0.5, -1.0, 1.0)
            steps[j].append(torch.from_numpy(sign * (mag if j == 0 else mag / 2)).float().reshape(shape))
    return params, steps


def plateau_scores():
    """A validation-score sequence with two plateaus for ReduceLROnPlateau(mode="max", patience=5): a rise, seven scores that are
    no improvement beyond the relative threshold (one of them above the best by less than 1e-4 of it), a rise, eight flat ones."""
    rise1 = [0.10, 0.30, 0.50, 0.60]
    flat1 = [0.60, 0.59, 0.60004, 0.55, 0.60, 0.58, 0.60]
    rise2 = [0.70, 0.80]
    flat2 = [0.80, 0.79, 0.80, 0.80, 0.78, 0.80, 0.80, 0.80]
    return rise1 + flat1 + rise2 + flat2
