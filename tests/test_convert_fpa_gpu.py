"""lidarnerf.convert's z-buffer ("fpa") and bbox-mask projections (csrc/convert.hip) against the reference's outputs
(tests/golden/g15_convert_fpa.npz: constructed clouds, so no pixel is left out) and the NumPy restatement of the rules
(tests/convert_fpa_ref.py).

Tolerance of the fpa values: 1 float32 ulp of float32(golden).  The device forms the same float64 sums as the reference (any
summation order differs by about 1e-15 relative) and rounds the quotient to float32 once; the bound is that rounding."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import convert_fpa_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FPA_CASES = ("a", "a_rev", "a_L1", "a_L2", "a_L16", "d")


@functools.lru_cache(maxsize=None)
def _g15():
    g = np.load(os.path.join(GOLD, "g15_convert_fpa.npz"))
    return {k: g[k] for k in g.files}, {c["name"]: c for c in json.loads(str(g["cases"]))}


def _cloud(g, c):
    return np.ascontiguousarray(g[c["cloud"]][::-1]) if c.get("reversed") else g[c["cloud"]]


def _assert_within_one_ulp(got, want, what):
    """got: float64 holding float32 values (the module's NumPy convention); want: the reference's float64 image."""
    got32, want32 = got.astype(np.float32), want.astype(np.float32)
    assert np.array_equal(got32.astype(np.float64), got), what  # the values ARE float32
    assert np.array_equal(got32 != 0, want32 != 0), (what, "zero / non-zero pattern")
    ulps = np.abs(got32.view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))
    print(f"{what}: max {ulps.max()} ulp, {(ulps > 0).sum()} of {(want32 != 0).sum()} pixels differ from float32(golden)")
    assert ulps.max() <= 1, (what, int(ulps.max()), np.argwhere(ulps > 1)[:5])


@pytest.mark.parametrize("name", FPA_CASES)
def test_fpa_matches_reference(name):
    from lidarnerf import convert
    g, cases = _g15()
    c = cases[name]
    pts, H, W, K = _cloud(g, c), c["H"], c["W"], tuple(c["K"])
    pano, inten = convert.lidar_to_pano_with_intensities_fpa(pts, H, W, K, max_depth=c["max_depth"],
                                                             z_buffer_len=c["z_buffer_len"])
    assert pano.dtype == np.float64 and pano.shape == (H, W) and inten.shape == (H, W)
    assert np.array_equal(pano != 0, inten != 0)
    _assert_within_one_ulp(pano, g[name + "_pano"], name + " pano")
    _assert_within_one_ulp(inten, g[name + "_inten"], name + " intensities")
    # a pixel with exactly one point: that point, bit for bit as the closest-point path gives it
    pix, _ = convert_fpa_ref.project(pts, H, W, K, c["max_depth"])
    single = (np.bincount(pix[pix >= 0], minlength=H * W) == 1).reshape(H, W)
    near, near_i = convert.lidar_to_pano_with_intensities(pts, H, W, K, max_depth=c["max_depth"])
    assert single.sum() >= 1
    assert np.array_equal(pano[single], near[single]) and np.array_equal(inten[single], near_i[single])
    assert np.array_equal(pano[single], g[name + "_pano"][single])


@pytest.mark.parametrize("n", (1, 255, 256, 257, 4099))
def test_fpa_point_counts_against_restatement(n):
    from lidarnerf import convert
    g, cases = _g15()
    c = cases["a"]
    pts, H, W, K = g["a_pts"][:n], c["H"], c["W"], tuple(c["K"])
    assert len(pts) == n
    want = convert_fpa_ref.lidar_to_pano_with_intensities_fpa(pts, H, W, K, c["max_depth"], 10)
    pano, inten = convert.lidar_to_pano_with_intensities_fpa(pts, H, W, K)  # (defaults: max_depth 80, z_buffer_len 10)
    _assert_within_one_ulp(pano, want[0], f"N={n} pano")
    _assert_within_one_ulp(inten, want[1], f"N={n} intensities")


def test_fpa_is_a_function_of_its_inputs():
    from lidarnerf import convert
    g, cases = _g15()
    for name in ("a", "d"):
        c = cases[name]
        t = torch.from_numpy(g[c["cloud"]]).cuda()
        first = convert.lidar_to_pano_with_intensities_fpa(t, c["H"], c["W"], tuple(c["K"]))
        again = convert.lidar_to_pano_with_intensities_fpa(t, c["H"], c["W"], tuple(c["K"]))
        assert first[0].is_cuda and first[1].is_cuda and first[0].dtype == torch.float32
        assert first[0].shape == (c["H"], c["W"])
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        host = convert.lidar_to_pano_with_intensities_fpa(g[c["cloud"]], c["H"], c["W"], tuple(c["K"]))
        assert np.array_equal(first[0].cpu().numpy(), host[0]) and np.array_equal(first[1].cpu().numpy(), host[1])


def test_fpa_edge_cases():
    from lidarnerf import convert
    H, W, K = 8, 16, (2.0, 26.9)
    p, i = convert.lidar_to_pano_with_intensities_fpa(np.zeros((0, 4), np.float32), H, W, K)
    assert p.shape == (H, W) and not p.any() and not i.any()
    # beyond max depth / above the field of view / at the sensor: every point dropped
    gone = np.array([[100.0, 0, 0, 0.5], [0, 0, 50.0, 0.5], [0, 0, 0, 0.5]], np.float32)
    p, i = convert.lidar_to_pano_with_intensities_fpa(gone, H, W, K)
    assert not p.any() and not i.any()
    p, i = convert.lidar_to_pano_with_intensities_fpa(torch.from_numpy(gone).cuda(), 66, 1030, K, z_buffer_len=1)
    assert p.is_cuda and not bool(p.any()) and not bool(i.any())
    for bad in (np.zeros((3, 3), np.float32), np.zeros((3, 5), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            convert.lidar_to_pano_with_intensities_fpa(bad, H, W, K)
    with pytest.raises(ValueError):
        convert.lidar_to_pano_with_intensities_fpa(gone, 0, W, K)
    with pytest.raises(RuntimeError, match="z_buffer_len"):
        convert.lidar_to_pano_with_intensities_fpa(gone, H, W, K, z_buffer_len=33)


@pytest.mark.parametrize("name", ("e0", "e1", "e2"))
def test_bbox_mask_matches_reference(name):
    from lidarnerf import convert
    g, cases = _g15()
    c = cases[name]
    H, W, K = c["H"], c["W"], tuple(c["K"])
    pano, inten = convert.lidar_to_pano_with_intensities_with_bbox_mask(g["e_pts"], H, W, K, g[name + "_bbox"],
                                                                        max_depth=c["max_depth"],
                                                                        max_intensity=c["max_intensity"])
    assert pano.dtype == np.float64 and pano.shape == (H, W)
    assert np.array_equal(pano, g[name + "_pano"]) and np.array_equal(inten, g[name + "_inten"])
    t, i = convert.lidar_to_pano_with_intensities_with_bbox_mask(torch.from_numpy(g["e_pts"]).cuda(), H, W, K,
                                                                 g[name + "_bbox"])
    assert t.is_cuda and i.is_cuda and t.dtype == torch.float32
    assert np.array_equal(t.cpu().numpy(), pano) and np.array_equal(i.cpu().numpy(), inten)


def test_bbox_mask_refusals():
    from lidarnerf import convert
    g, cases = _g15()
    c = cases["e0"]
    H, W, K = c["H"], c["W"], tuple(c["K"])
    up = np.array([[0.0, 0.0, 5.0, 1.0]] * 8)  # every corner straight above the sensor: none lands in the image
    with pytest.raises(ValueError, match="no corner"):
        convert.lidar_to_pano_with_intensities_with_bbox_mask(g["e_pts"], H, W, K, up)
    with pytest.raises(ValueError):
        convert.lidar_to_pano_with_intensities_with_bbox_mask(np.zeros((3, 3), np.float32), H, W, K, g["e0_bbox"])
