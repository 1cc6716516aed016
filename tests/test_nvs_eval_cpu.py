"""The NVS baselines' evaluation without a GPU: the lnh_nvs_eval_* entry points against the header and the binding, their
argument checks (made before any launch), the workspace size, the Python surface of lidarnerf/nvs_eval.py with its refusals, and
the restatement tests/nvs_eval_ref.py — its two modes against each other within derived bounds, its 1-D SSIM against a direct
uniform_filter + crop formulation and the exact rational evaluation, and the rectangle addressing against run.py's crop."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import nvs_eval_ref as ref

INVALID_ARG, UNSUPPORTED = -1, -2  # LNH_ERR_INVALID_ARG, LNH_ERR_UNSUPPORTED (include/lidarnerf_hip.h)
ENTRY_POINTS = ("lnh_nvs_eval_frame", "lnh_nvs_eval_ssim", "lnh_nvs_eval_finalize")
TILE = 256  # positions per workgroup of the SSIM kernel (kNvsTile, csrc/nvs_ssim_tile.h)


def test_exports_header_and_signatures():
    from lidarnerf import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "lidarnerf_hip.h")).read()
    slots = dict((n.lower(), int(v)) for n, v in re.findall(r"LNH_NVS_(\w+) = (\d+)", text))
    assert slots.pop("slots") == _hip.NVS_SLOTS == 18
    names = [k for k, _ in sorted(slots.items(), key=lambda kv: kv[1])]
    names = ["f_score" if n == "fscore" else n for n in names]  # (the reference's key has the underscore)
    assert names == list(_hip.NVS_SLOT_NAMES)
    assert _hip.NVS_METRICS == ("depth_rmse", "depth_a1", "depth_a2", "depth_a3", "depth_ssim", "intensity_mae", "chamfer", "f_score")
    assert _hip.NVS_METRICS[:6] == ref.METRICS
    L = _hip.lib()
    for name in ENTRY_POINTS:
        assert name in _hip._SIGS and name in _hip.EXPORTS and name in _hip._OPTIONAL and hasattr(L, name)
        assert re.search(r"LNH_API int " + name + r"\(", text)
        assert getattr(L, name).argtypes[-1] is C.c_void_p  # (the stream)
    assert "lnh_nvs_eval_workspace_bytes" in _hip.EXPORTS and re.search(r"LNH_API uint64_t lnh_nvs_eval_workspace_bytes\(", text)
    assert L.lnh_nvs_eval_workspace_bytes.restype is C.c_uint64
    assert L.lnh_version() == 102  # (the new entry points are detected by symbol)
    src = open(os.path.join(root, "lidar-nerf_amd", "csrc", "nvs_ssim_tile.h")).read()
    assert re.search(r"kNvsTile = (\d+)", src).group(1) == str(TILE)


def test_workspace_size():
    from lidarnerf import _hip
    L = _hip.lib()
    for H, W in ((1, 1), (1, 7), (1, 8), (3, 5), (6, 16), (23, 37), (1, TILE + 6), (1, TILE + 7), (66, 1030), (4096, 4096)):
        N = H * W
        tiles = max(1, -(-max(N - 6, 0) // TILE))
        assert L.lnh_nvs_eval_workspace_bytes(H, W) == -(-N // 1024) * 64 + tiles * 8, (H, W)
    for H, W in ((0, 5), (5, 0), (4096, 4097), (1 << 16, 1 << 16)):
        assert L.lnh_nvs_eval_workspace_bytes(H, W) == 0


def test_entry_points_check_arguments_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    H, W = 23, 37
    need = L.lnh_nvs_eval_workspace_bytes(H, W)
    buf = (C.c_double * (need // 8 + 2))()
    ws = (C.addressof(buf) + 7) & ~7
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced

    def frame(gp=x, pp=x, gi=x, pi=x, mask=None, h=H, w=W, s=1.0, wsp=ws, wsb=need):
        return L.lnh_nvs_eval_frame(gp, pp, gi, pi, mask, h, w, s, wsp, wsb, None)

    for kw, word in ((dict(gp=None), "pano"), (dict(pp=None), "pano"), (dict(gi=None), "intensity"), (dict(pi=None), "intensity"),
                     (dict(gp=18), "aligned"), (dict(pi=17), "aligned"), (dict(h=0), "at least 1"), (dict(w=0), "at least 1"),
                     (dict(s=0.0), "intensity_scale"), (dict(s=-255.0), "intensity_scale"), (dict(s=math.inf), "intensity_scale"),
                     (dict(s=math.nan), "intensity_scale"), (dict(wsp=None), "workspace"), (dict(wsb=need - 8), "workspace"),
                     (dict(wsp=ws + 4), "workspace"), (dict(h=66, w=1030), "workspace")):
        assert frame(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert frame(h=4096, w=4097) == UNSUPPORTED and "2^24" in err()

    def ssim(gp=x, pp=x, mask=None, h=H, w=W, wsp=ws, wsb=need):
        return L.lnh_nvs_eval_ssim(gp, pp, mask, h, w, wsp, wsb, None)

    for kw, word in ((dict(gp=None), "pano"), (dict(pp=None), "pano"), (dict(pp=18), "aligned"), (dict(h=0), "at least 1"),
                     (dict(w=0), "at least 1"), (dict(wsp=None), "workspace"), (dict(wsb=need - 8), "workspace"),
                     (dict(wsp=ws + 4), "workspace")):
        assert ssim(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert ssim(h=4096, w=4097) == UNSUPPORTED and "2^24" in err()

    def finalize(h=H, w=W, wsp=ws, wsb=need, row=x, acc=x, hist=x, frames=4):
        return L.lnh_nvs_eval_finalize(h, w, wsp, wsb, row, acc, hist, frames, None)

    for kw, word in ((dict(row=None), "points_row"), (dict(acc=None), "accumulator"), (dict(hist=None), "history"),
                     (dict(row=12), "aligned"), (dict(acc=12), "aligned"), (dict(hist=20), "aligned"), (dict(h=0), "at least 1"),
                     (dict(wsp=None), "workspace"), (dict(wsb=need - 8), "workspace")):
        assert finalize(**kw) == INVALID_ARG and word in err(), (kw, err())
    assert finalize(h=4096, w=4097) == UNSUPPORTED and "2^24" in err()


def test_python_surface_and_refusals():
    from lidarnerf import nvs, nvs_eval
    for name in ("NVSFrameEvaluator", "eval_points_and_pano", "evaluate_nvs", "FieldNVS"):
        assert getattr(nvs, name) is getattr(nvs_eval, name)
    sig = inspect.signature(nvs_eval.NVSFrameEvaluator.__init__)
    assert list(sig.parameters)[1:7] == ["H", "W", "intrinsics", "nerf_mvl", "threshold", "max_frames"]
    assert sig.parameters["nerf_mvl"].default is False and sig.parameters["threshold"].default == 0.05
    assert sig.parameters["max_frames"].default == 1024
    assert list(inspect.signature(nvs_eval.NVSFrameEvaluator.update).parameters)[1:] == ["gt_frame", "pd_frame"]
    for name in ("rows", "measure", "report", "clear"):
        assert callable(getattr(nvs_eval.NVSFrameEvaluator, name))
    p = inspect.signature(nvs_eval.evaluate_nvs).parameters
    assert list(p)[:4] == ["nvs", "frames", "raydrop", "nerf_mvl"] and p["raydrop"].default is True and p["nerf_mvl"].default is False
    assert list(p.values())[-1].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(nvs_eval.FieldNVS.__init__).parameters
    assert list(p)[1:] == ["trainer", "scale", "ema"] and p["ema"].default is True
    assert list(inspect.signature(nvs_eval.FieldNVS.predict_frame_with_raydrop).parameters)[1:] == \
        ["lidar_K", "lidar_pose", "lidar_H", "lidar_W"]
    for cls in (nvs.MeshNVS, nvs.PointCloudNVS):
        assert list(inspect.signature(cls.evaluate).parameters)[1:4] == ["frames", "raydrop", "nerf_mvl"]
        assert list(inspect.signature(cls.predict_images_with_raydrop).parameters)[1:5] == ["lidar_K", "lidar_pose", "lidar_H", "lidar_W"]

    H, W = 6, 16
    ev = nvs_eval.NVSFrameEvaluator(H, W, (2.0, 26.9))
    assert ev.intensity_scale == 1.0 and nvs_eval.NVSFrameEvaluator(H, W, (2.0, 26.9), nerf_mvl=True).intensity_scale == 255.0
    frame = {"pano": torch.zeros(H, W), "intensities": torch.zeros(H, W)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(frame, frame)
    with pytest.raises(RuntimeError, match="no frame"):
        ev.measure()
    with pytest.raises(RuntimeError, match="no frame"):
        ev.rows()
    ev.clear()  # (nothing to clear yet: not an error)
    for bad in (dict(H=0), dict(W=-1), dict(max_frames=-1), dict(points_capacity=0), dict(threshold=0.0)):
        kw = dict(H=H, W=W, intrinsics=(2.0, 26.9))
        kw.update(bad)
        with pytest.raises(ValueError):
            nvs_eval.NVSFrameEvaluator(**kw)
    with pytest.raises(ValueError, match="scale"):
        nvs_eval.FieldNVS(object(), 0.0)
    with pytest.raises(ValueError, match="no frames"):
        nvs_eval.evaluate_nvs(object(), [])


def test_eval_points_and_pano_checks_its_arguments_like_the_reference():
    from lidarnerf.nvs import eval_points_and_pano
    assert list(inspect.signature(eval_points_and_pano).parameters) == [
        "gt_local_points", "pd_local_points", "gt_intensities", "pd_intensities", "gt_pano", "pd_pano"]
    H, W = 6, 16
    pts, img = np.zeros((5, 3), np.float32), np.zeros((H, W), np.float32)
    good = dict(gt_local_points=pts, pd_local_points=pts, gt_intensities=img, pd_intensities=img, gt_pano=img, pd_pano=img)
    for key, value, message in (
            ("gt_local_points", np.zeros((5, 4), np.float32), "gt_local_points must be (N, 3), but got (5, 4)"),
            ("gt_local_points", np.zeros(5, np.float32), "gt_local_points must be (N, 3), but got (5,)"),
            ("pd_local_points", np.zeros((3, 5, 3), np.float32), "pd_local_points must be (M, 3), but got (3, 5, 3)"),
            ("gt_intensities", np.zeros(H * W, np.float32), f"gt_intensities must be (H, W), but got ({H * W},)"),
            ("pd_intensities", img[:, :-1], f"pd_intensities must be (H, W), but got ({H}, {W - 1})"),
            ("gt_pano", img[:-1], f"gt_pano must be (H, W), but got ({H - 1}, {W})"),
            ("pd_pano", img.T, f"pd_pano must be (H, W), but got ({W}, {H})"),
            ("pd_pano", torch.zeros(H, W), "All inputs must be numpy array.")):
        kw = dict(good)
        kw[key] = value
        with pytest.raises(ValueError) as info:
            eval_points_and_pano(**kw)
        assert str(info.value) == message
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            eval_points_and_pano(**good)


def _frame(H, W, seed, exact=False):
    rng = np.random.default_rng(seed)
    if exact:
        gt = rng.choice(np.array([0, 1, 2, 4, 5, 8, 10, 16, 1000], np.float32), (H, W))
        pd = rng.choice(np.array([0, 1, 2, 4, 5, 8, 10, 16, 1000], np.float32), (H, W))
        gi, pi = (rng.integers(0, 17, (H, W)) / 16).astype(np.float32), (rng.integers(0, 17, (H, W)) / 16).astype(np.float32)
    else:
        gt, pd = rng.uniform(0, 90, (H, W)).astype(np.float32), rng.uniform(0, 90, (H, W)).astype(np.float32)
        drop = rng.random((H, W)) < 0.1
        gt[drop], pd[rng.random((H, W)) < 0.1] = 0, 0
        gi, pi = rng.random((H, W), np.float32), rng.random((H, W), np.float32)
    return gt, pd, gi, pi


@pytest.mark.parametrize("H,W,masked", [(23, 37, False), (23, 37, True), (66, 1030, False), (1, 7, False), (3, 5, False)])
def test_the_two_modes_differ_by_float32_rounding_only(H, W, masked):
    """faithful against contract.  The sums: np.mean of n non-negative float32 terms in float32 is off by at most n 2^-24
    relative (any summation order), and so the means; sqrt halves a relative error and rounds once more.  The SSIM: both
    modes within their running error bounds of the exact rational S (ssim_error_bounds: unit roundoff 2^-24 through
    uniform_filter for faithful, 2^-53 for contract), per position and for the mean.  Counts and n are integers: equal."""
    gt, pd, gi, pi = _frame(H, W, 5)
    mask = None
    if masked:
        mask = np.zeros((H, W), bool)
        mask[3:19, 5:30] = True
    f, c = ref.evaluate(gt, pd, gi, pi, mask, "faithful"), ref.evaluate(gt, pd, gi, pi, mask, "contract")
    n = c["n"]
    assert f["n"] == n == (16 * 25 if masked else H * W) and f["counts"] == c["counts"] and f["data_range"] == c["data_range"]
    for key in ("depth_a1", "depth_a2", "depth_a3"):
        assert f[key] == c[key]
    rel = n * ref.U32
    assert abs(f["intensity_mae"] - c["intensity_mae"]) <= (rel + 2 * ref.U32) * c["intensity_mae"]
    assert abs(f["depth_rmse"] - c["depth_rmse"]) <= (rel / 2 + 3 * ref.U32) * c["depth_rmse"]
    if masked:
        assert c["intensity_mae"] > 20  # (the crop multiplies by 255)
    g, p = ref.clamp(ref.crop_frame(gt, pd, gi, pi, mask)[0]), ref.clamp(ref.crop_frame(gt, pd, gi, pi, mask)[1])
    if n > 2000:  # (the rational model is slow: the small shapes carry it)
        assert abs(f["depth_ssim"] - c["depth_ssim"]) < 1e-4
        return
    exact = ref.ssim_exact(g, p, c["data_range"])
    assert len(exact) == n - 6 == c["S"].size == f["S"].size and None not in exact
    b64 = ref.ssim_error_bounds(g, p, c["data_range"], ref.U64)
    b32 = ref.ssim_error_bounds(g, p, c["data_range"], ref.U32, filtered=True)
    e64 = np.array([abs(float(ref.Fraction(float(s)) - e)) for s, e in zip(c["S"], exact)])
    e32 = np.array([abs(float(ref.Fraction(float(s)) - e)) for s, e in zip(f["S"], exact)])
    print(f"{H} x {W}: contract uses {np.max(e64 / b64):.3g} of its bound, faithful {np.max(e32 / b32):.3g} "
          f"(largest bounds {b64.max():.3g}, {b32.max():.3g})")
    assert np.all(np.isfinite(b64)) and np.all(e64 <= b64)
    assert np.all(e32 <= b32)  # (an infinite bound — a denominator the float32 error can reach — holds nothing)
    mean = float(sum(exact) / len(exact))
    s_abs = float(sum(abs(e) for e in exact))
    assert abs(c["depth_ssim"] - mean) <= ref.mean_bound(s_abs, b64)
    if np.all(np.isfinite(b32)):
        assert abs(f["depth_ssim"] - mean) <= ref.mean_bound(s_abs, b32)


@pytest.mark.parametrize("n", [7, 8, 15, 96, TILE + 6, 851])
def test_contract_ssim_against_a_direct_uniform_filter_formulation(n):
    """The restated kernel arithmetic against skimage's algorithm run in float64 (uniform_filter over the whole signal, then the
    crop by 3 on either side): the same positions, each within the sum of the two running error bounds."""
    rng = np.random.default_rng(n)
    x, y = ref.clamp(rng.uniform(0, 90, n)), ref.clamp(rng.uniform(0, 90, n))
    R = ref.data_range(x)
    S = ref.ssim_contract(x, y, R)
    D, mean = ref.ssim_uniform_filter(x, y, R, dtype=np.float64)
    assert S.shape == D.shape == (n - 6,)
    bound = ref.ssim_error_bounds(x, y, R, ref.U64) + ref.ssim_error_bounds(x, y, R, ref.U64, filtered=True)
    assert np.all(np.abs(S - D) <= bound) and bound.max() < 1e-9
    assert abs(mean - math.fsum(S.tolist()) / (n - 6)) <= bound.max() + 1e-15
    # identical signals: unfused products make the numerator and the denominator the same bits
    assert np.all(ref.ssim_contract(x, x, R) == 1.0)
    assert ref.ssim_contract(x[:6], y[:6], R).size == 0 and math.isnan(ref.ssim_uniform_filter(x[:6], y[:6], R)[1])


def _rectangle(mask):
    """The kernel's integer reduction: (r0, c0, h, w, count) of a mask."""
    rows, cols = np.nonzero(mask)
    if rows.size == 0:
        return 0, 0, 0, 0, 0
    return int(rows.min()), int(cols.min()), int(rows.max() - rows.min() + 1), int(cols.max() - cols.min() + 1), int(rows.size)


def test_rectangle_addressing_equals_the_boolean_index_and_reshape():
    """run.py:209-217 takes image[mask] and reshapes it to the bounding rectangle; the kernels address element p of that
    sequence as (r0 + p / w, c0 + p % w).  Equal for every mask that fills its rectangle; the reference raises for one that
    does not, where the count differs from h * w."""
    H, W = 23, 37
    image = np.arange(H * W, dtype=np.float32).reshape(H, W)
    for r0, c0, h, w in ((0, 0, 5, 9), (0, 28, 5, 9), (18, 0, 5, 9), (18, 28, 5, 9), (4, 3, 1, 7), (0, 0, H, W), (7, 7, 2, 3), (22, 36, 1, 1)):
        mask = np.zeros((H, W), bool)
        mask[r0:r0 + h, c0:c0 + w] = True
        assert _rectangle(mask) == (r0, c0, h, w, h * w)
        want = ref.crop(image, mask)
        p = np.arange(h * w)
        got = image[r0 + p // w, c0 + p % w]
        assert want.shape == (h, w) and np.array_equal(want.flatten(), got)
    ell = np.zeros((H, W), bool)
    ell[2:6, 3] = ell[5, 3:9] = True
    r0, c0, h, w, count = _rectangle(ell)
    assert (r0, c0, h, w, count) == (2, 3, 4, 6, 9) and count != h * w
    with pytest.raises(ValueError):
        ref.crop(image, ell)
    with pytest.raises(ValueError):
        ref.crop(image, np.zeros((H, W), bool))
    assert _rectangle(np.zeros((H, W), bool)) == (0, 0, 0, 0, 0)


def test_exact_images_have_exact_terms():
    """The exact tier's premise: on depths from {0, 1, 2, 4, 5, 8, 10, 16, 1000} and intensities k / 16 every square and every
    absolute difference is a dyadic rational that float32 holds, so their sum is the same in any order and precision."""
    gt, pd, gi, pi = _frame(23, 37, 3, exact=True)
    g, p, thresh, sq, ad = ref.terms(gt, pd, gi * 255, pi * 255)
    assert math.fsum(sq.tolist()) == float(sq.astype(np.float64).sum()) == float(np.sum(sq[::-1], dtype=np.float64))
    assert math.fsum(ad.tolist()) * 16 == round(math.fsum(ad.tolist()) * 16)
    assert set(np.unique(g)) <= {np.float32(1e-3), 1, 2, 4, 5, 8, 10, 16, 80}
    # pairs exactly on a threshold stay out of the strict comparison, in both directions
    for k, (a, b) in enumerate(((5, 4), (25, 16), (62.5, 32))):  # (125 / 64 as 62.5 / 32: 125 would be clamped to 80)
        for x, y in ((a, b), (b, a)):
            t = ref.terms(np.float32([[x]]), np.float32([[y]]), np.float32([[0]]), np.float32([[0]]))[2][0]
            assert float(t) == ref.THRESHOLDS[k] and [bool(t < s) for s in ref.THRESHOLDS] == [j > k for j in range(3)]
