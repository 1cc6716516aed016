"""NumPy restatement of what lnh_lidar_sample_batch draws (csrc/lidar_sample.hip): Philox-4x32-10 (Salmon et al., SC'11;
pinned by the published Random123 known answer for the all-zero counter and key), the range mapping (uint64(r) * m) >> 32, the
index layout of a batch, and — in float64 — the ray directions."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KAT_ZERO = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)  # Random123 kat_vectors: philox4x32 10, counter 0, key 0
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32-valued arrays (broadcastable), key: two -> four uint64 arrays holding the 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = (np.uint64(int(v) & 0xFFFFFFFF) for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c


def to_range(r, m):
    return (np.asarray(r, dtype=np.uint64) * np.uint64(m)) >> np.uint64(32)


def batch_rows(N, H, W, px, py):
    n = min(N, H * W)
    return n // (px * py) * (px * py) if px > 0 else n


def corners(N, H, W, px, py, seed, draw, stream_id):
    """Top-left (rows, cols) of the patches of draw number `draw` (px > 0)."""
    num_patch = batch_rows(N, H, W, px, py) // (px * py)
    w = philox4x32_10((np.arange(num_patch), draw & 0xFFFFFFFF, draw >> 32, stream_id), (seed & 0xFFFFFFFF, seed >> 32))
    return to_range(w[0], H - px).astype(np.int64), to_range(w[1], W - py).astype(np.int64)


def batch_indices(N, H, W, px, py, seed, draw, stream_id):
    """inds [n] of draw number `draw`: patches back to back, px rows x py columns row-major inside a patch."""
    if px <= 0:
        n = batch_rows(N, H, W, px, py)
        w = philox4x32_10((np.arange(n), draw & 0xFFFFFFFF, draw >> 32, stream_id), (seed & 0xFFFFFFFF, seed >> 32))
        return to_range(w[0], H * W).astype(np.int64)
    rows, cols = corners(N, H, W, px, py, seed, draw, stream_id)
    k = np.arange(px * py)
    r = rows[:, None] + (k // py)[None, :]
    c = cols[:, None] + (k % py)[None, :]
    return (r * W + c).reshape(-1)


def directions(inds, pose, H, W, fov_up, fov):
    """rays_d [n,3] in float64: R (cos a cos b, cos a sin b, sin a), b = -(col - W/2)/W 2 pi, a = (fov_up - row/H fov) pi/180."""
    inds = np.asarray(inds, dtype=np.int64)
    row, col = (inds // W).astype(np.float64), (inds % W).astype(np.float64)
    beta = -(col - W / 2.0) / W * 2.0 * np.pi
    alpha = (float(fov_up) - row / H * float(fov)) / 180.0 * np.pi
    d = np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.sin(alpha)], -1)
    return d @ np.asarray(pose, dtype=np.float64)[:3, :3].T
