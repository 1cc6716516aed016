"""NumPy restatement of the z-buffer ("fpa") and bbox-mask projections of the reference's lidarnerf/convert.py (4-97, 253-361),
as rules on the SET of points of a pixel rather than as the reference's per-point replay.  tests/golden/g15_convert_fpa.npz holds
the reference's own outputs; this file is what the device kernels (csrc/convert.hip) are compared with at other point counts.

fpa, for a pixel that received n points, L = z_buffer_len, threshold = 0.2:
    n == 0        (0, 0)
    n == 1        that point's (dist, intensity)
    2 <= n <= L   the buffer is in arrival (point index) order; parse_z_buffer's slice [1:n] leaves out the LAST-arrived point
    n > L         the buffer holds the L smallest under (dist, point index); the slice leaves out the largest of them
                  (L == 1: the smallest point itself, parse_z_buffer's `z_buffer_num == 1` branch)
    of what remains, the points with d <= d_min + threshold (float64 on float32 depths) are averaged with weights 1 / d.
"""
import numpy as np

THRESHOLD = 0.2


def project(points, H, W, K, max_depth=80):
    """Per point: row-major pixel id (-1 = dropped by the max-depth or bounds test), and the float32 distances."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    fov_up, fov = K
    fov_down = fov - fov_up
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    dists = np.linalg.norm(pts[:, :3], axis=1)  # float32, like the reference's
    beta = np.float32(np.pi) - np.arctan2(y, x)
    alpha = np.arctan2(z, np.sqrt(x**2 + y**2)) + np.float32(fov_down / 180 * np.pi)
    c = np.rint(beta / np.float32(2 * np.pi / W)).astype(np.int64)              # Python round(): half to even
    r = np.rint(np.float32(H) - alpha / np.float32(fov / 180 * np.pi / H)).astype(np.int64)
    ok = (dists < max_depth) & (dists > 0) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
    return np.where(ok, r * W + c, -1), dists


def _buckets(pix):
    """pixel id -> point indices in ascending order."""
    idx = np.nonzero(pix >= 0)[0]
    order = idx[np.argsort(pix[idx], kind="stable")]
    ids, starts = np.unique(pix[order], return_index=True)
    return ids, np.split(order, starts[1:])


def lidar_to_pano_with_intensities_fpa(points, H, W, K, max_depth=80, z_buffer_len=10, threshold=THRESHOLD):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    pix, dists = project(pts, H, W, K, max_depth)
    L = int(z_buffer_len)
    pano, inten = np.zeros(H * W), np.zeros(H * W)
    if not (pix >= 0).any():
        return pano.reshape(H, W), inten.reshape(H, W)
    for p, idx in zip(*_buckets(pix)):
        n = len(idx)
        if n > L:
            idx = idx[np.lexsort((idx, dists[idx]))][:L]  # the L smallest under (dist, index), in that order
        if len(idx) == 1:
            pano[p], inten[p] = dists[idx[0]], pts[idx[0], 3]
            continue
        idx = idx[:-1]
        d = dists[idx].astype(np.float64)
        keep = d <= d.min() + threshold
        d, i = d[keep], pts[idx, 3].astype(np.float64)[keep]
        pano[p] = np.average(d, weights=1 / d)
        inten[p] = np.average(i, weights=1 / d)
    return pano.reshape(H, W), inten.reshape(H, W)


def bbox_window(bbox_local, H, W, K):
    """(r_min, r_max, c_min, c_max) of the box corners that land in the image (maxima exclusive, as the reference's slice is);
    None when no corner does."""
    fov_up, fov = K
    fov_down = fov - fov_up
    rs, cs = [], []
    for x, y, z, _ in np.asarray(bbox_local):
        beta = np.pi - np.arctan2(y, x)
        alpha = np.arctan2(z, np.sqrt(x**2 + y**2)) + fov_down / 180 * np.pi
        c = int(round(beta / (2 * np.pi / W)))
        r = int(round(H - alpha / (fov / 180 * np.pi / H)))
        if 0 <= r < H and 0 <= c < W:
            rs.append(r)
            cs.append(c)
    return (min(rs), max(rs), min(cs), max(cs)) if rs else None


def lidar_to_pano_with_intensities_with_bbox_mask(points, H, W, K, bbox_local, max_depth=80, max_intensity=255.0):
    """Pixels are independent: the closest point ((dist, index) minimum) inside the window, -1 outside it."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    win = bbox_window(bbox_local, H, W, K)
    if win is None:
        raise ValueError("no corner of bbox_local lands in the image")
    r0, r1, c0, c1 = win
    pix, dists = project(pts, H, W, K, max_depth)
    pano, inten = np.full((H, W), -1.0), np.zeros((H, W))
    pano[r0:r1, c0:c1] = 0
    if (pix >= 0).any():
        for p, idx in zip(*_buckets(pix)):
            r, c = divmod(int(p), W)
            if pano[r, c] < 0:
                continue
            k = idx[np.lexsort((idx, dists[idx]))][0]
            pano[r, c] = dists[k]
            inten[r, c] = pts[k, 3] / np.float32(max_intensity)
    return pano, inten
