"""NumPy / SciPy restatement of the NVS baselines' evaluation, written from the semantics of lidarnvs/eval.py:9-135
(eval_points_and_pano's depth and intensity metrics) and of the NeRF-MVL crop of lidarnvs/run.py:200-217.  Two modes:

faithful   float32 NumPy as the reference computes — in-place clamps of flattened copies, np.mean of float32 arrays in
           float32, data_range a float32 difference — and the SSIM from skimage.metrics.structural_similarity's published
           algorithm on float32 signals with scipy.ndimage.uniform_filter (the filter skimage itself calls), NumPy 2 scalar
           promotion.  Unpinned vs a real scikit-image build: the package is not installed, this is its algorithm restated.
contract   the same float32 per-pixel terms; sums in fp64 (math.fsum: the exact sum, rounded once); the SSIM with the
           arithmetic of csrc/nvs_ssim_tile.h — window moments as fp64 sums of the 7 float32 values from left to right, S in
           fp64, one rounded operation per operator.  What lnh_nvs_eval_* promise.

ssim_exact evaluates the same S with fractions.Fraction, and ssim_error_bounds carries a running rounding-error bound through
the formula (every operation's result off by at most u times its magnitude, on top of what its operands carry): the bounds
the tests hold both modes and the kernel to.  The point metrics are tests/eval_points_ref.py's."""
import math
from fractions import Fraction

import numpy as np
from scipy.ndimage import uniform_filter

WIN, K1, K2 = 7, 0.01, 0.03
MIN_DEPTH, MAX_DEPTH = np.float32(1e-3), np.float32(80)
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
U32, U64 = 2.0 ** -24, 2.0 ** -53
METRICS = ("depth_rmse", "depth_a1", "depth_a2", "depth_a3", "depth_ssim", "intensity_mae")


def crop(image, pano_mask):
    """run.py:209-217 for one image: the masked pixels in row-major order, reshaped to their bounding rectangle (raises
    where they do not fill it, as the reference does)."""
    idx = np.array(np.nonzero(pano_mask))
    new_h = max(idx[0]) - min(idx[0]) + 1
    new_w = max(idx[1]) - min(idx[1]) + 1
    return image[pano_mask].reshape(new_h, new_w)


def crop_frame(gt_pano, pd_pano, gt_int, pd_int, pano_mask=None):
    """The four images as eval_points_and_pano receives them: cropped and the intensities times 255 with a mask."""
    if pano_mask is None:
        return gt_pano, pd_pano, gt_int, pd_int
    pano_mask = np.asarray(pano_mask) != 0
    return (crop(gt_pano, pano_mask), crop(pd_pano, pano_mask), crop(gt_int, pano_mask) * 255, crop(pd_int, pano_mask) * 255)


def clamp(depths):
    """eval.py:81-84 on a flattened float32 copy."""
    d = np.array(depths, dtype=np.float32).flatten()
    d[d < MIN_DEPTH] = MIN_DEPTH
    d[d > MAX_DEPTH] = MAX_DEPTH
    return d


def terms(gt_pano, pd_pano, gt_int, pd_int):
    """The float32 per-pixel terms both modes share: clamped depths, thresh, (gt - pd)^2, |gt_i - pd_i|."""
    gt, pd = clamp(gt_pano), clamp(pd_pano)
    with np.errstate(all="ignore"):
        thresh = np.maximum(gt / pd, pd / gt)
        sq = (gt - pd) ** 2
        ad = np.abs(np.asarray(gt_int, np.float32) - np.asarray(pd_int, np.float32)).flatten()
    assert thresh.dtype == sq.dtype == ad.dtype == np.float32
    return gt, pd, thresh, sq, ad


def data_range(gt):
    return gt.max() - gt.min()  # float32


def ssim_uniform_filter(x, y, R, dtype=np.float32):
    """skimage's algorithm on 1-D signals: per-position S over the positions whose window lies inside (the crop by
    (win - 1) // 2), and their float64 mean."""
    if x.size < WIN:
        return np.zeros(0), float("nan")
    x, y = x.astype(dtype), y.astype(dtype)
    cov_norm = WIN / (WIN - 1)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    R = dtype(R)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    with np.errstate(all="ignore"):
        A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
        S = (A1 * A2) / (B1 * B2)
    pad = (WIN - 1) // 2
    S = S[pad:S.size - pad]
    return S, float(S.mean(dtype=np.float64))


def ssim_constants(R):
    R = float(R)
    return (K1 * R) * (K1 * R), (K2 * R) * (K2 * R)


def ssim_contract(x, y, R):
    """csrc/nvs_ssim_tile.h in NumPy fp64, operation for operation: per-position S [n - 6]."""
    n = x.size
    if n < WIN:
        return np.zeros(0)
    m = n - (WIN - 1)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    sx, sy, sxx, syy, sxy = (np.zeros(m) for _ in range(5))
    for j in range(WIN):
        a, b = xd[j:j + m], yd[j:j + m]
        sx, sy, sxx, syy, sxy = sx + a, sy + b, sxx + a * a, syy + b * b, sxy + a * b
    npix = float(WIN)
    cov_norm = npix / (npix - 1.0)
    ux, uy, uxx, uyy, uxy = sx / npix, sy / npix, sxx / npix, syy / npix, sxy / npix
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = ssim_constants(R)
    with np.errstate(all="ignore"):
        a1, a2 = 2.0 * ux * uy + c1, 2.0 * vxy + c2
        b1, b2 = ux * ux + uy * uy + c1, vx + vy + c2
        return (a1 * a2) / (b1 * b2)


def ssim_exact(x, y, R):
    """Per-position S as exact rationals of the float32 inputs (K1, K2 the doubles 0.01 and 0.03, the covariance norm 7 / 6):
    a list of Fractions, None where the denominator is 0."""
    X, Y = [Fraction(float(v)) for v in x], [Fraction(float(v)) for v in y]
    R = Fraction(float(R))
    C1, C2 = (Fraction(K1) * R) ** 2, (Fraction(K2) * R) ** 2
    norm = Fraction(WIN, WIN - 1)
    px, py = [0], [0]
    pxx, pyy, pxy = [0], [0], [0]
    for a, b in zip(X, Y):
        px.append(px[-1] + a), py.append(py[-1] + b)
        pxx.append(pxx[-1] + a * a), pyy.append(pyy[-1] + b * b), pxy.append(pxy[-1] + a * b)
    out = []
    for q in range(len(X) - WIN + 1):
        ux, uy = (px[q + WIN] - px[q]) / WIN, (py[q + WIN] - py[q]) / WIN
        uxx, uyy, uxy = (pxx[q + WIN] - pxx[q]) / WIN, (pyy[q + WIN] - pyy[q]) / WIN, (pxy[q + WIN] - pxy[q]) / WIN
        vx, vy, vxy = norm * (uxx - ux * ux), norm * (uyy - uy * uy), norm * (uxy - ux * uy)
        den = (ux * ux + uy * uy + C1) * (vx + vy + C2)
        out.append(((2 * ux * uy + C1) * (2 * vxy + C2)) / den if den != 0 else None)
    return out


class _E:
    """A value with a bound on its absolute error; every operation adds u times the magnitude of its result (one rounding)
    to what its operands carry, to first order plus the product of the operands' errors."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = v, e


def _add(a, b, u, sign=1.0):
    v = a.v + sign * b.v
    return _E(v, a.e + b.e + u * np.abs(v))


def _mul(a, b, u):
    v = a.v * b.v
    return _E(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + u * np.abs(v))


def _div(a, b, u):
    with np.errstate(all="ignore"):
        v = a.v / b.v
        room = np.abs(b.v) - b.e
        e = np.where(room > 0, (a.e + np.abs(v) * b.e) / np.where(room > 0, room, 1.0), np.inf) + u * np.abs(v)
    return _E(v, e)


def ssim_error_bounds(x, y, R, u, filtered=False):
    """Bound on |computed S - exact S| per position [n - 6] for an evaluation that rounds every operation to unit roundoff u
    (2^-53: the kernel and the contract mode; 2^-24: the faithful mode).  filtered=False: the window moments are sums of the
    7 terms from left to right, rounded after every addition, of products rounded once.  filtered=True: the moments come from
    uniform_filter — a sliding sum in double along the whole line (each of its n steps adds and subtracts one term: at most
    (2 n + 16) 2^-53 times the largest term, the first window's seven additions and the division included), divided by 7 and rounded to the signal's precision u, of products rounded to u.
    Magnitudes are taken from the fp64 evaluation (a relative 2^-50 of the bound, covered by the factor at the end)."""
    n = x.size
    m = n - (WIN - 1)
    xd, yd = x.astype(np.float64), y.astype(np.float64)

    def moment(t, t_err):  # t: the n terms (fp64 values), t_err: their error bounds
        win = np.lib.stride_tricks.sliding_window_view(t, WIN)
        mean_abs = np.abs(win).sum(1) / WIN
        err_terms = np.lib.stride_tricks.sliding_window_view(t_err, WIN).sum(1) / WIN
        mean = win.sum(1) / WIN
        if filtered:
            return _E(mean, err_terms + (2.0 * n + 16.0) * U64 * np.abs(t).max() + u * mean_abs)
        return _E(mean, err_terms + (WIN + 1) * u * mean_abs)  # 6 additions and the division: (1 + u)^7 - 1 <= 8 u

    zero = np.zeros(n)
    ux, uy = moment(xd, zero), moment(yd, zero)
    uxx, uyy, uxy = moment(xd * xd, u * xd * xd), moment(yd * yd, u * yd * yd), moment(xd * yd, u * np.abs(xd * yd))
    norm = _E(WIN / (WIN - 1.0), u * WIN / (WIN - 1.0))
    vx = _mul(norm, _add(uxx, _mul(ux, ux, u), u, -1.0), u)
    vy = _mul(norm, _add(uyy, _mul(uy, uy, u), u, -1.0), u)
    vxy = _mul(norm, _add(uxy, _mul(ux, uy, u), u, -1.0), u)
    c1v, c2v = ssim_constants(R)
    c1, c2 = _E(c1v, 6 * u * c1v), _E(c2v, 6 * u * c2v)  # (K R)^2: K rounded to the signal's precision, two or three products
    two = _E(2.0)
    a1 = _add(_mul(_mul(two, ux, u), uy, u), c1, u)
    a2 = _add(_mul(two, vxy, u), c2, u)
    b1 = _add(_add(_mul(ux, ux, u), _mul(uy, uy, u), u), c1, u)
    b2 = _add(_add(vx, vy, u), c2, u)
    S = _div(_mul(a1, a2, u), _mul(b1, b2, u), u)
    assert S.v.shape == (m,)
    return S.e * (1.0 + 2.0 ** -20)


def mean_bound(S_abs_sum, per_position_bounds, u=U64):
    """Bound on |computed mean - exact mean| of m values summed in any order in precision u and divided once."""
    m = per_position_bounds.size
    gamma = m * u / (1.0 - m * u)
    return (float(per_position_bounds.sum()) + gamma * S_abs_sum) / m + u * S_abs_sum / m


def evaluate(gt_pano, pd_pano, gt_int, pd_int, pano_mask=None, mode="contract"):
    """The six image metrics of eval_points_and_pano for one frame (after run.py's crop with a pano_mask), plus the pieces the
    tests compare: n, counts, sum_sq, sum_abs, data_range and the per-position S."""
    gt_pano, pd_pano, gt_int, pd_int = crop_frame(gt_pano, pd_pano, gt_int, pd_int, pano_mask)
    gt, pd, thresh, sq, ad = terms(gt_pano, pd_pano, gt_int, pd_int)
    n = gt.size
    R = data_range(gt)
    counts = [int((thresh < t).sum()) for t in THRESHOLDS]
    out = {"n": n, "counts": counts, "data_range": float(R), "depth_a1": counts[0] / n, "depth_a2": counts[1] / n,
           "depth_a3": counts[2] / n}
    if mode == "faithful":
        out["depth_rmse"] = float(np.sqrt(sq.mean()))
        out["intensity_mae"] = float(ad.mean())
        assert sq.mean().dtype == np.float32
        out["S"], out["depth_ssim"] = ssim_uniform_filter(gt, pd, R)
    else:
        out["sum_sq"], out["sum_abs"] = math.fsum(sq.tolist()), math.fsum(ad.tolist())
        out["depth_rmse"] = math.sqrt(out["sum_sq"] / n)
        out["intensity_mae"] = out["sum_abs"] / n
        out["S"] = ssim_contract(gt, pd, R)
        out["depth_ssim"] = math.fsum(out["S"].tolist()) / (n - WIN + 1) if n >= WIN else float("nan")
    return out
