#!/usr/bin/env python3
"""G15: the reference's lidar_to_pano_with_intensities_fpa and lidar_to_pano_with_intensities_with_bbox_mask
(lidarnerf/convert.py:253-361, 4-97) on constructed clouds (CPU).

    python tests/golden/make_g15_convert_fpa.py <reference checkout>

Writes g15_convert_fpa.npz next to this script.  The clouds are CONSTRUCTED: every point targets a pixel (r, c) with an angular
jitter of at most +-0.35 pixel, and the script asserts
  * in float64, every point's unrounded row and column coordinate is at least 0.1 away from a half-integer;
  * the reference's own (r, c) — its closest-point function called on the single point — equals the target;
  * inside a pixel distinct depths differ by at least 1e-4, no difference of two depths lies within 1e-4 of the 0.2 m
    threshold, and exact duplicates are bit-identical points (x, y, z),
so no last-bit difference in atan2 or sqrt can move a point or flip a selection: a test of these vectors leaves out no pixel.
Equal depths and np.argsort.  The reference replays an overflowing buffer through np.argsort's DEFAULT kind.  That sort is stable
for these sizes in NumPy's scalar code, but NumPy 2 dispatches it to a vectorised sort on CPUs with AVX2 / AVX-512, which is not:
there the reference's answer on a pixel with equal depths depends on the CPU it runs on.  The rule the device implements is the
stable one (equal depths resolve towards the earlier point), so this script runs the reference's two functions with `np.argsort`
bound to kind="stable" inside the reference's module, and changes nothing else.  It also runs them as they are and asserts that
every pixel WITHOUT two equal depths comes out bit-identical either way.  tests/convert_fpa_ref.py restates the rules; it is
asserted equal to every stored output bit for bit.

Cases (arrays `<case>_pts`, `<case>_pano`, `<case>_inten`; `cases` is a JSON list of their parameters):
  a      8 x 16, intrinsics (2.0, 26.9), z_buffer_len 10: per-pixel counts 0, 1, 2, 9, 10, 11, 63..65, 255..257 and 1300; ties of
         equal depth with different intensities at the selection boundaries; points at or beyond max_depth (one at exactly 80.0)
         and outside the field of view; peaks wider than 0.2 m.  (A little over 4099 points: the device tests take prefixes.)
  a_rev  the same cloud reversed (pins the last-arrival rule); stores no cloud of its own
  a_L1, a_L2, a_L16   cloud a at other z_buffer_len
  d      66 x 1030, most pixels empty (the scan spans several chunks)
  e0..e2 bbox mask on 32 x 64, intrinsics (15, 40): a box inside the image, a box with corners outside it, a box whose window is
         empty (r_min == r_max); one cloud `e_pts`, intensities 0..255, boxes `e<k>_bbox`
"""
import argparse
import importlib.util
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEP = 0.003  # depth lattice inside a pixel: 0.2 / STEP is 66.67, so no two lattice depths are 0.2 m apart


class _StableArgsortNumpy:
    """numpy, with argsort's default kind replaced by "stable" (module docstring)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kw):
        kw.setdefault("kind", "stable")
        return np.argsort(a, *args, **kw)


def load_reference(root, stable_argsort=False):
    spec = importlib.util.spec_from_file_location("ref_convert", os.path.join(root, "lidarnerf", "convert.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if stable_argsort:
        mod.np = _StableArgsortNumpy()
    return mod


def point(r, c, jr, jc, d, H, W, K):
    """float64 point at distance d whose unrounded image coordinates are (r + jr, c + jc)."""
    fov_up, fov = K
    beta = (c + jc) * 2 * np.pi / W
    alpha = (H - (r + jr)) * (fov / 180 * np.pi / H)
    az, el = np.pi - beta, alpha - (fov - fov_up) / 180 * np.pi
    return d * np.cos(el) * np.cos(az), d * np.cos(el) * np.sin(az), d * np.sin(el)


class Cloud:
    def __init__(self, H, W, K, seed):
        self.H, self.W, self.K, self.rng = H, W, K, np.random.default_rng(seed)
        self.rows, self.target = [], []

    def add(self, r, c, d, intensity=None, jitter=None):
        jr, jc = self.rng.uniform(-0.35, 0.35, 2) if jitter is None else jitter
        jc = abs(jc) if c == 0 else jc  # (column 0 is half a pixel wide: beta < 0 wraps round to column W)
        x, y, z = point(r, c, jr, jc, d, self.H, self.W, self.K)
        i = self.rng.uniform(0, 1) if intensity is None else intensity
        self.rows.append(np.array([x, y, z, i], dtype=np.float32))
        self.target.append((r, c))

    def duplicate(self, intensity):
        """The last point again, bit for bit, with another intensity."""
        row = self.rows[-1].copy()
        row[3] = intensity
        self.rows.append(row)
        self.target.append(self.target[-1])

    def pixel(self, r, c, n, base, span):
        """n points on the depth lattice base + k * STEP, k distinct in [0, span)."""
        for k in self.rng.choice(span, size=n, replace=False):
            self.add(r, c, base + k * STEP)

    def finish(self):
        pts, tgt = np.stack(self.rows), np.array(self.target)
        perm = self.rng.permutation(len(pts))  # arrival order is unrelated to pixel and depth
        return pts[perm], tgt[perm]


def check(ref, pts, tgt, H, W, K, max_depth=80):
    """The generator's three assertions (module docstring)."""
    fov_up, fov = K
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    u = (np.pi - np.arctan2(y, x)) / (2 * np.pi / W)
    v = H - (np.arctan2(z, np.sqrt(x**2 + y**2)) + (fov - fov_up) / 180 * np.pi) / (fov / 180 * np.pi / H)
    for coord in (u, v):
        assert np.all(np.abs(coord - np.floor(coord) - 0.5) >= 0.1), "a point sits within 0.1 pixel of a pixel boundary"
    dists = np.linalg.norm(pts[:, :3], axis=1)
    inside = (tgt[:, 0] >= 0) & (tgt[:, 0] < H) & (tgt[:, 1] >= 0) & (tgt[:, 1] < W)
    for k in range(len(pts)):
        pano, _ = ref.lidar_to_pano_with_intensities(pts[k:k + 1], H, W, K, max_depth=np.inf)
        hit = np.argwhere(pano != 0)
        if inside[k]:
            assert len(hit) == 1 and tuple(hit[0]) == tuple(tgt[k]), (k, hit, tgt[k])
        else:
            assert len(hit) == 0, (k, hit, tgt[k])
    pix = np.where(inside & (dists < max_depth), tgt[:, 0] * W + tgt[:, 1], -1)
    for p in np.unique(pix[pix >= 0]):
        idx = np.nonzero(pix == p)[0]
        d = dists[idx].astype(np.float64)
        diff = np.abs(d[:, None] - d[None, :])
        same = diff == 0
        assert np.all(diff[~same] >= 1e-4), "two depths of a pixel are closer than 1e-4"
        assert np.all(np.abs(diff - 0.2) >= 1e-4), "a depth difference lies within 1e-4 of the threshold"
        for a, b in np.argwhere(same):
            assert np.array_equal(pts[idx[a], :3], pts[idx[b], :3]), "equal depths must be bit-identical points"
    return np.bincount(pix[pix >= 0], minlength=H * W)


def tied_pixels(pts, H, W, K, max_depth=80):
    """[H * W] bool: pixels that hold two points of equal depth."""
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    import convert_fpa_ref
    pix, dists = convert_fpa_ref.project(pts, H, W, K, max_depth)
    tied = np.zeros(H * W, bool)
    for p in np.unique(pix[pix >= 0]):
        d = dists[pix == p]
        tied[p] = len(np.unique(d)) < len(d)
    return tied


def cloud_a():
    H, W, K = 8, 16, (2.0, 26.9)
    cl = Cloud(H, W, K, 15)
    free = [(r, c) for r in range(H) for c in range(W)]
    cl.rng.shuffle(free)
    free = [tuple(int(v) for v in f) for f in free]
    free.remove((0, 0))  # (0, 0) stays empty; so does one more pixel below
    empty = free.pop()
    for n in (1, 2, 9, 10, 11, 63, 64, 65, 255, 256, 257):
        r, c = free.pop()
        cl.pixel(r, c, n, cl.rng.uniform(5, 60), n * 3 + 5 if n % 2 else n * 40 + 100)
    r, c = free.pop()
    cl.pixel(r, c, 1300, 12.0, 3000)
    # ties (bit-identical points, other intensity) at sorted positions (a, a + 1) of 14 points: around z_buffer_len 10
    # (8|9 kept/left out, 9|10 in/out of the buffer), the minimum (0|1), and around z_buffer_len 1, 2 (1|2)
    for a in (8, 9, 0, 1):
        r, c = free.pop()
        base = cl.rng.uniform(5, 60)
        ks = np.sort(cl.rng.choice(120, size=13, replace=False))
        order = cl.rng.permutation(13)
        for j in order:
            cl.add(r, c, base + ks[j] * STEP)
            if j == a:
                cl.duplicate(cl.rng.uniform(0, 1))
    # 20 points in 4 groups of 5 equal depths (z_buffer_len 16 cuts the last group)
    r, c = free.pop()
    for g in range(4):
        cl.add(r, c, 30.0 + 17 * g * STEP)
        for _ in range(4):
            cl.duplicate(cl.rng.uniform(0, 1))
    # peaks wider than 0.2 m: 9 and 25 points 0.06 m apart
    for n in (9, 25):
        r, c = free.pop()
        for k in cl.rng.permutation(n):
            cl.add(r, c, 20.0 + 20 * k * STEP)
    # at and beyond max_depth, in a pixel that also has nearer points; one point at exactly 80.0
    r, c = free.pop()
    for d in (79.5, 79.9, 80.5, 95.0, 300.0):
        cl.add(r, c, d)
    for _ in range(10000):
        cl.add(r, c, 80.0)
        if np.linalg.norm(cl.rows[-1][:3]) == np.float32(80.0):
            break
        cl.rows.pop(), cl.target.pop()
    else:
        raise AssertionError("no point at exactly 80.0")
    r, c = free.pop()
    cl.add(r, c, 120.0)  # a pixel whose only point is too far: stays empty
    # outside the field of view: above, below, and the column that rounds to W
    for rr, cc, j in ((-1, 3, None), (-3, 9, None), (H, 5, None), (H + 2, 12, None), (4, W, (0.1, -0.3)), (2, W, (-0.2, -0.15))):
        cl.add(rr, cc, 25.0, jitter=j)
    for r, c in free:
        n = int(cl.rng.integers(1, 36))
        cl.pixel(r, c, n, cl.rng.uniform(3, 70), n * 3 + 5 if cl.rng.uniform() < 0.5 else n * 40 + 100)
    pts, tgt = cl.finish()
    return H, W, K, pts, tgt, empty


def cloud_d():
    H, W, K = 66, 1030, (2.0, 26.9)
    cl = Cloud(H, W, K, 16)
    chosen = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (3, 1001), (3, 1002)}  # corners; two neighbours
    while len(chosen) < 1500:
        chosen.add((int(cl.rng.integers(H)), int(cl.rng.integers(W))))
    for r, c in sorted(chosen):
        n = int(min(cl.rng.geometric(0.14), 40))
        cl.pixel(r, c, n, cl.rng.uniform(3, 70), n * 3 + 5 if cl.rng.uniform() < 0.5 else n * 40 + 100)
    for _ in range(60):
        cl.add(int(cl.rng.integers(H)), int(cl.rng.integers(W)), cl.rng.uniform(81, 200))
        cl.add(int(cl.rng.choice([-2, -1, H, H + 1])), int(cl.rng.integers(W)), 30.0)
    pts, tgt = cl.finish()
    return H, W, K, pts, tgt


def cloud_e():
    H, W, K = 32, 64, (15.0, 40.0)
    cl = Cloud(H, W, K, 17)
    for r in range(H):
        for c in range(W):
            n = int(cl.rng.choice([0, 0, 1, 1, 2]))
            if n:
                cl.pixel(r, c, n, cl.rng.uniform(3, 70), 400)
    for _ in range(30):
        cl.add(int(cl.rng.integers(H)), int(cl.rng.integers(W)), cl.rng.uniform(81, 200))
        cl.add(int(cl.rng.choice([-2, -1, H, H + 1])), int(cl.rng.integers(W)), 30.0)
    pts, tgt = cl.finish()
    pts[:, 3] = np.where(cl.rng.uniform(size=len(pts)) < 0.5, cl.rng.integers(0, 256, len(pts)),
                         cl.rng.uniform(0, 255, len(pts))).astype(np.float32)
    pts[:3, 3] = (0.0, 255.0, 1.0)

    def box(targets):
        rows = []
        for r, c in targets:
            jr, jc = cl.rng.uniform(-0.35, 0.35, 2)
            rows.append(list(point(r, c, jr, jc, cl.rng.uniform(5, 30), H, W, K)) + [1.0])
        return np.array(rows, dtype=np.float64)

    boxes = [box([(8, 12), (8, 40), (20, 12), (20, 40), (10, 15), (10, 37), (18, 15), (18, 37)]),
             box([(-3, 50), (-1, 60), (5, 50), (5, 61), (25, 52), (25, 58), (H + 2, 52), (H, 58)]),
             box([(14, 5), (14, 9), (14, 30), (14, 22), (14, 17), (14, 11), (-2, 3), (H + 1, 40)])]
    windows = [(8, 20, 12, 40), (5, 25, 50, 61), (14, 14, 5, 30)]
    return H, W, K, pts, tgt, boxes, windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference project")
    a = ap.parse_args()
    ref, ref_as_is = load_reference(a.reference, stable_argsort=True), load_reference(a.reference)
    out, cases = {}, []

    def fpa(name, cloud, pts, H, W, K, L):
        pano, inten = ref.lidar_to_pano_with_intensities_fpa(pts, H, W, K, max_depth=80, z_buffer_len=L)
        pano2, inten2 = ref_as_is.lidar_to_pano_with_intensities_fpa(pts, H, W, K, max_depth=80, z_buffer_len=L)
        untied = ~tied_pixels(pts, H, W, K).reshape(H, W)
        assert np.array_equal(pano[untied], pano2[untied]) and np.array_equal(inten[untied], inten2[untied]), name
        out[name + "_pano"], out[name + "_inten"] = pano, inten
        cases.append(dict(name=name, kind="fpa", cloud=cloud, reversed=name.endswith("_rev"), H=H, W=W, K=list(K), max_depth=80,
                          z_buffer_len=L))

    H, W, K, pts, tgt, empty = cloud_a()
    counts = check(ref, pts, tgt, H, W, K)
    assert len(pts) > 4099 and counts[0] == 0 and counts[empty[0] * W + empty[1]] == 0
    assert set((0, 1, 2, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1300)) <= set(counts.tolist())
    assert (np.linalg.norm(pts[:, :3], axis=1) == np.float32(80.0)).sum() == 1
    out["a_pts"] = pts
    fpa("a", "a_pts", pts, H, W, K, 10)
    fpa("a_rev", "a_pts", pts[::-1], H, W, K, 10)
    assert np.abs(out["a_rev_pano"] - out["a_pano"]).max() > 0.01  # the order matters
    for L in (1, 2, 16):
        fpa(f"a_L{L}", "a_pts", pts, H, W, K, L)

    H, W, K, pts, tgt = cloud_d()
    counts = check(ref, pts, tgt, H, W, K)
    assert (counts == 0).mean() > 0.9 and counts.max() > 10
    out["d_pts"] = pts
    fpa("d", "d_pts", pts, H, W, K, 10)

    H, W, K, pts, tgt, boxes, windows = cloud_e()
    check(ref, pts, tgt, H, W, K)
    out["e_pts"] = pts
    for k, (bbox, win) in enumerate(zip(boxes, windows)):
        pano, inten = ref.lidar_to_pano_with_intensities_with_bbox_mask(pts, H, W, K, bbox, max_depth=80, max_intensity=255.0)
        r0, r1, c0, c1 = win
        mask = np.zeros((H, W), bool)
        mask[r0:r1, c0:c1] = True
        assert np.array_equal(pano == -1, ~mask), (k, win)  # the window is the intended one (every pixel outside it is -1)
        assert k == 2 or ((pano > 0).sum() > 20 and (inten > 0).sum() > 20)
        out[f"e{k}_bbox"], out[f"e{k}_pano"], out[f"e{k}_inten"] = bbox, pano, inten
        cases.append(dict(name=f"e{k}", kind="bbox", cloud="e_pts", H=H, W=W, K=list(K), max_depth=80, max_intensity=255.0,
                          window=list(win)))
    import convert_fpa_ref
    for c in cases:  # the restatement of the rules (tests/convert_fpa_ref.py) equals the reference bit for bit
        pts = out[c["cloud"]][::-1] if c.get("reversed") else out[c["cloud"]]
        if c["kind"] == "fpa":
            got = convert_fpa_ref.lidar_to_pano_with_intensities_fpa(pts, c["H"], c["W"], c["K"], 80, c["z_buffer_len"])
        else:
            got = convert_fpa_ref.lidar_to_pano_with_intensities_with_bbox_mask(pts, c["H"], c["W"], c["K"],
                                                                                out[c["name"] + "_bbox"], 80, 255.0)
        assert np.array_equal(got[0], out[c["name"] + "_pano"]) and np.array_equal(got[1], out[c["name"] + "_inten"]), c["name"]
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "g15_convert_fpa.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB, clouds a {len(out['a_pts'])} d {len(out['d_pts'])} "
          f"e {len(out['e_pts'])} points")


if __name__ == "__main__":
    main()
