"""NumPy float64 restatement of the ray-drop MLP contract of csrc/raydrop.hip (include/lidarnerf_hip.h, lnh_raydrop_*): forward,
loss, gradients (normalised once: the backward carries 2 (out - t) or sign(out - t), every weight and bias gradient is its sum
over the batch divided by B at the end) and torch.optim.Adam.  tests/test_raydrop_cpu.py asserts it equal to the float64 tensors of
G16 (the reference's own module cast to double) to 1e-12 relative.

Also the integer-valued problems of the exact known-answer tests: every product and every sum of them is an integer below 2^24, so
each output has ONE right fp32 value whatever the order of the sums."""
import numpy as np

IN = 5


def param_count(D, W):
    return W * IN + W + (D - 1) * (W * W + W) + W + 1


def split(params, D, W):
    """[(weight [out, in], bias [out])] * (D + 1): views of the flat buffer in torch's order."""
    layers, o = [], 0
    for l in range(D + 1):
        rows, cols = (W, IN if l == 0 else W) if l < D else (1, W)
        w = params[o:o + rows * cols].reshape(rows, cols)
        o += rows * cols
        layers.append((w, params[o:o + rows]))
        o += rows
    assert o == len(params) == param_count(D, W)
    return layers


def forward(params, D, W, x, keep=False):
    """x [N, 5] -> out [N] (and the activations of every hidden layer with keep=True)."""
    layers = split(params, D, W)
    h, acts = x, []
    for w, b in layers[:-1]:
        h = np.maximum(h @ w.T + b, 0)
        acts.append(h)
    out = (h @ layers[-1][0].T + layers[-1][1]).reshape(-1)
    return (out, acts) if keep else out


def loss_and_grad(params, D, W, rows, loss_type, parts=None):
    """rows [B, 6] -> out [B], the loss numerator sum_i e_i, loss = numerator / B, grad [P] (each sum over the batch / B).
    parts (a dict): receives the unnormalised sums `gsum` [P] and the per-layer dY and activations."""
    layers = split(params, D, W)
    B = rows.shape[0]
    x, t = rows[:, :IN], rows[:, IN]
    out, acts = forward(params, D, W, x, keep=True)
    d = out - t
    if loss_type == 0:
        e, g = d * d, 2 * d
    else:
        e, g = np.abs(d), np.sign(d)
    gsum = np.zeros_like(params)
    gl = split(gsum, D, W)
    dys = [None] * D
    gl[D][0][:] = g[None, :] @ acts[-1]
    gl[D][1][:] = g.sum()
    dy = (g[:, None] * layers[D][0]) * (acts[-1] > 0)
    for l in range(D - 1, -1, -1):
        dys[l] = dy
        gl[l][0][:] = dy.T @ (acts[l - 1] if l > 0 else x)
        gl[l][1][:] = dy.sum(axis=0)
        if l > 0:
            dy = (dy @ layers[l][0]) * (acts[l - 1] > 0)
    if parts is not None:
        parts.update(gsum=gsum, dys=dys, acts=acts, dout=g, e=e)
    return out, e.sum(), e.sum() / B, gsum / B


def adam(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One torch.optim.Adam step (no weight decay, no amsgrad); t: the step count BEFORE this step.  Returns p, m, v."""
    t = t + 1
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps
    return p - (lr / (1 - beta1 ** t)) * m / denom, m, v


# ------------------------------------------------------------------------------------------------- exact integer problems
EXACT_SHAPES = [(1, 128), (2, 128), (4, 128), (8, 256), (3, 256)]
# The row tile of k_raydrop_rows is 16 and the weight-gradient kernel deals rows to four waves in chunks of 4 * ceil(B / 16), 32
# rows per loop trip (rows behind a chunk's end are masked): 1, 15, 16, 17 sit on either side of one row tile, 63, 64, 65 of four
# tiles and of a wave chunk of 16 (half a trip), 127, 128, 129 of a wave chunk of exactly one trip, 257 is seventeen tiles with a one-row tail — wave chunks of 68 rows (three trips,
# the last one partial) and a last chunk of 53 rows, an odd number of 4-row MFMA steps.
EXACT_SIZES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257]
LIMIT = 1 << 24


def exact_case(D, W, B, loss_type, seed=0):
    """Integer-valued parameters [P] and rows [B, 6] (float64 arrays).  Hidden matrices have three entries of +-1 per row at
    random columns (asymmetric: a transposed or permuted operand reads other values), biases in -1 .. 2, inputs in small ranges;
    half the targets lie within 2 of the output, a fifth of those on it (the L1 gradient's 0 at 0)."""
    rng = np.random.default_rng(1000 * D + W + 7 * seed)
    params = np.zeros(param_count(D, W))
    layers = split(params, D, W)
    layers[0][0][:] = rng.integers(-1, 2, (W, IN))
    for l in range(1, D):
        w = layers[l][0]
        for j in range(W):
            w[j, rng.choice(W, 3, replace=False)] = rng.choice([-1, 1], 3)
    for l in range(D):
        layers[l][1][:] = rng.integers(-1, 3, W)
    wo = layers[D][0][0]
    wo[rng.choice(W, 12, replace=False)] = rng.choice([-1, 1], 12)
    layers[D][1][:] = 1
    rows = np.zeros((B, 6))
    rows[:, :3] = rng.integers(-1, 2, (B, 3))
    rows[:, 3] = rng.integers(0, 4, B)
    rows[:, 4] = rng.integers(0, 3, B)
    out = forward(params, D, W, rows[:, :IN])
    rows[:, 5] = rng.integers(0, 2, B)
    near = rng.uniform(size=B) < 0.5  # half the targets are 0 / 1, half lie within 2 of the output (both signs and 0)
    rows[near, 5] = out[near] + rng.integers(-2, 3, int(near.sum()))
    return params, rows


def exact_bound(params, D, W, rows, loss_type):
    """The largest sum of ABSOLUTE products over every dot product of forward, backward, weight gradients and the loss: below
    2^24 means every partial sum in every order is an exactly representable integer."""
    ap = np.abs(params)
    parts = {}
    loss_and_grad(params, D, W, rows, loss_type, parts)
    layers = split(ap, D, W)
    x = np.abs(rows[:, :IN])
    acts = [np.abs(a) for a in parts["acts"]]
    dys = [np.abs(d) for d in parts["dys"]]
    worst = 0.0
    h = x
    for l in range(D):
        worst = max(worst, (h @ layers[l][0].T + layers[l][1]).max())
        h = acts[l]
    worst = max(worst, (h @ layers[D][0].T + layers[D][1]).max() + np.abs(rows[:, IN]).max())
    worst = max(worst, parts["e"].sum(), 2 * np.abs(parts["dout"]).max())
    g = np.abs(parts["dout"])
    worst = max(worst, (g[None, :] @ acts[-1]).max(), g.sum())
    for l in range(D - 1, -1, -1):
        worst = max(worst, (dys[l].T @ (acts[l - 1] if l > 0 else x)).max(), dys[l].sum(axis=0).max())
        if l > 0:
            worst = max(worst, (dys[l] @ layers[l][0]).max())
    return worst
