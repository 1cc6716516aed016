"""The z-buffer ("fpa") and bbox-mask conversions without a GPU: the three entry points are exported, declared and bound; every
refusal of lnh_lidar_to_pano_fpa / lnh_lidar_to_pano_masked happens before any launch; the NumPy restatement of the rules
(tests/convert_fpa_ref.py) equals the reference's outputs (tests/golden/g15_convert_fpa.npz) bit for bit; and the Python functions
keep the reference's parameter names."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import convert_fpa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, UNSUPPORTED = -1, -2  # LNH_ERR_INVALID_ARG, LNH_ERR_UNSUPPORTED (include/lidarnerf_hip.h)
NAMES = ("lnh_lidar_to_pano_fpa", "lnh_lidar_to_pano_fpa_workspace_size", "lnh_lidar_to_pano_masked")


def _g15():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g15_convert_fpa.npz"))
    return g, json.loads(str(g["cases"]))


def test_entry_points_are_exported_declared_and_bound():
    from lidarnerf import _hip
    text = open(os.path.join(ROOT, "include", "lidarnerf_hip.h")).read()
    L = _hip.lib()
    for name in NAMES:
        assert name in _hip.EXPORTS and hasattr(L, name), name
        assert re.search(r"LNH_API (int|uint64_t) " + name + r"\(", text), name
    assert "Replaces lidar_to_pano_with_intensities_fpa" in text
    assert "Replaces lidar_to_pano_with_intensities_with_bbox_mask" in text
    P, U32, U64, F32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    assert _hip._SIGS["lnh_lidar_to_pano_fpa"] == [P, U64, U32, U32, F32, F32, F32, U32, C.c_double, P, U64, P, P]
    assert _hip._SIGS["lnh_lidar_to_pano_masked"] == [P, U32, U32, U32, F32, F32, F32, U32, U32, U32, U32, F32, P, P, P]
    assert L.lnh_lidar_to_pano_fpa.argtypes == _hip._SIGS["lnh_lidar_to_pano_fpa"] + [P]
    assert L.lnh_lidar_to_pano_masked.argtypes == _hip._SIGS["lnh_lidar_to_pano_masked"] + [P]
    assert L.lnh_lidar_to_pano_fpa_workspace_size.restype is U64
    assert L.lnh_lidar_to_pano_fpa_workspace_size.argtypes == [U64, U32, U32]


def test_workspace_size_grows_with_points_and_pixels():
    from lidarnerf import _hip
    size = _hip.lib().lnh_lidar_to_pano_fpa_workspace_size
    base = size(1000, 8, 16)
    assert base >= 1000 * 12 + 8 * 16 * 12 and size(0, 8, 16) > 0
    assert size(1001, 8, 16) > base or size(1002, 8, 16) > base  # (rounded up to 16 bytes)
    assert size(2000, 8, 16) >= base + 12000 and size(1000, 66, 1030) >= base + (66 * 1030 - 128) * 12
    assert size(5_000_000, 66, 1030) < 1 << 27
    for n, h, w in ((10, 0, 16), (10, 8, 0), (10, 1 << 13, (1 << 11) + 1), (1 << 32, 8, 16)):
        assert size(n, h, w) == 0
    assert size(10, 1 << 12, 1 << 12) > 0 and size((1 << 32) - 1, 8, 16) > 0


def test_every_refusal_comes_before_any_launch():
    from lidarnerf import _hip
    L = _hip.lib()
    err = lambda: L.lnh_last_error().decode()
    N, H, W = 100, 8, 16
    need = L.lnh_lidar_to_pano_fpa_workspace_size(N, H, W)
    x = 16  # any non-null, aligned value: every call below must fail before it is dereferenced

    def fpa(pts=x, n=N, h=H, w=W, fov=26.9, L_=10, th=0.2, ws=x, wsb=need, pano=x, inten=x):
        return L.lnh_lidar_to_pano_fpa(pts, n, h, w, 2.0, fov, 80.0, L_, th, ws, wsb, pano, inten, None)

    for kw, word in ((dict(pts=None), "null"), (dict(pano=None), "null"), (dict(inten=None), "null"), (dict(h=0), "image size"),
                     (dict(w=0), "image size"), (dict(fov=0.0), "fov"), (dict(fov=-1.0), "fov"), (dict(th=-0.1), "threshold"),
                     (dict(ws=None), "workspace"), (dict(wsb=need - 8), "workspace"), (dict(ws=20), "workspace"),
                     (dict(n=N + 4096), "workspace")):  # (more points need a larger workspace)
        assert fpa(**kw) == INVALID_ARG and word in err(), (kw, err())
    for kw, word in ((dict(L_=0), "z_buffer_len"), (dict(L_=33), "z_buffer_len"), (dict(h=1 << 13, w=(1 << 11) + 1), "2^24"),
                     (dict(n=1 << 32), "32 bits")):
        assert fpa(**kw) == UNSUPPORTED and word in err(), (kw, err())

    def masked(pts=x, n=N, h=H, w=W, fov=26.9, win=(2, 6, 3, 9), keys=x, pano=x, inten=x):
        return L.lnh_lidar_to_pano_masked(pts, n, h, w, 2.0, fov, 80.0, *win, 255.0, keys, pano, inten, None)

    for kw, word in ((dict(pts=None), "null"), (dict(keys=None), "null"), (dict(pano=None), "null"), (dict(inten=None), "null"),
                     (dict(h=0), "image size"), (dict(w=0), "image size"), (dict(fov=0.0), "fov"),
                     (dict(win=(6, 2, 3, 9)), "window"), (dict(win=(2, 9, 3, 9)), "window"), (dict(win=(2, 6, 9, 3)), "window"),
                     (dict(win=(2, 6, 3, 17)), "window")):
        assert masked(**kw) == INVALID_ARG and word in err(), (kw, err())


def test_restatement_equals_the_reference_bit_for_bit():
    g, cases = _g15()
    assert [c["name"] for c in cases] == ["a", "a_rev", "a_L1", "a_L2", "a_L16", "d", "e0", "e1", "e2"]
    for c in cases:
        pts = g[c["cloud"]][::-1] if c.get("reversed") else g[c["cloud"]]
        if c["kind"] == "fpa":
            pano, inten = convert_fpa_ref.lidar_to_pano_with_intensities_fpa(pts, c["H"], c["W"], c["K"], c["max_depth"],
                                                                            c["z_buffer_len"])
        else:
            pano, inten = convert_fpa_ref.lidar_to_pano_with_intensities_with_bbox_mask(
                pts, c["H"], c["W"], c["K"], g[c["name"] + "_bbox"], c["max_depth"], c["max_intensity"])
            r0, r1, c0, c1 = c["window"]
            assert convert_fpa_ref.bbox_window(g[c["name"] + "_bbox"], c["H"], c["W"], c["K"]) == (r0, r1, c0, c1)
            assert (pano == -1).sum() == c["H"] * c["W"] - (r1 - r0) * (c1 - c0)
        want_pano, want_inten = g[c["name"] + "_pano"], g[c["name"] + "_inten"]
        assert pano.dtype == want_pano.dtype == np.float64
        assert np.array_equal(pano, want_pano) and np.array_equal(inten, want_inten), c["name"]


def test_fixture_covers_what_it_claims():
    g, cases = _g15()
    a = cases[0]
    pix, dists = convert_fpa_ref.project(g["a_pts"], a["H"], a["W"], a["K"], a["max_depth"])
    counts = np.bincount(pix[pix >= 0], minlength=a["H"] * a["W"])
    assert {0, 1, 2, 9, 10, 11, 63, 64, 65, 255, 256, 257} <= set(counts.tolist()) and counts.max() > 1000
    assert len(g["a_pts"]) > 4099 and (dists == np.float32(80.0)).sum() == 1 and (dists > 80).sum() >= 4
    assert (pix < 0).sum() >= 11  # too far or outside the field of view
    assert np.abs(g["a_rev_pano"] - g["a_pano"]).max() > 0.01  # the order of the points matters
    for name in ("a_L1", "a_L2", "a_L16"):
        assert not np.array_equal(g[name + "_pano"], g["a_pano"])
    d = cases[5]
    assert (d["H"], d["W"]) == (66, 1030) and (g["d_pano"] == 0).mean() > 0.9
    assert [(g[f"e{k}_pano"] == -1).all() for k in range(3)] == [False, False, True]
    assert g["e_pts"][:, 3].max() == 255.0 and g["e0_inten"].max() <= 1.0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_convert_fpa.npz")) < 1 << 20


def test_python_surface_and_no_cpu_fallback():
    from lidarnerf import convert
    sig = inspect.signature(convert.lidar_to_pano_with_intensities_fpa)
    assert list(sig.parameters) == ["local_points_with_intensities", "lidar_H", "lidar_W", "lidar_K", "max_depth", "z_buffer_len"]
    assert sig.parameters["max_depth"].default == 80 and sig.parameters["z_buffer_len"].default == 10
    sig = inspect.signature(convert.lidar_to_pano_with_intensities_with_bbox_mask)
    assert list(sig.parameters) == ["local_points_with_intensities", "lidar_H", "lidar_W", "lidar_K", "bbox_local", "max_depth",
                                    "max_intensity"]
    assert sig.parameters["max_depth"].default == 80 and sig.parameters["max_intensity"].default == 255.0
    assert "Not built" not in convert.__doc__ and convert.FPA_THRESHOLD == 0.2
    pts = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        convert.lidar_to_pano_with_intensities_fpa(pts, 8, 16, (2.0, 26.9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        convert.lidar_to_pano_with_intensities_with_bbox_mask(pts, 8, 16, (2.0, 26.9), np.ones((8, 4)))
    g, cases = _g15()
    e = cases[6]
    assert convert._bbox_window(g["e0_bbox"], e["H"], e["W"], e["K"]) == tuple(e["window"])
    assert convert._bbox_window(torch.from_numpy(g["e2_bbox"]), e["H"], e["W"], e["K"]) == tuple(cases[8]["window"])
    with pytest.raises(ValueError, match="no corner"):
        convert._bbox_window(np.array([[0.0, 0.0, 5.0, 1.0]] * 8), e["H"], e["W"], e["K"])  # straight up: above the image
    with pytest.raises(ValueError):
        convert._bbox_window(np.ones((8, 3)), e["H"], e["W"], e["K"])
