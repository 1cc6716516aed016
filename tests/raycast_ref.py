"""NumPy float32 restatement of the ray-casting contract of csrc/raycast.hip (include/lidarnerf_hip.h, lnh_raycast_*): the
watertight intersection function in the stated operation order (float64 recomputation of the edge functions when one is
exactly 0 included), the minimum key over ALL triangles, normals and incidences.  Vectorised over rays x triangles, in chunks
of rays.  Plus the ray sets and the grid geometry the tests share."""
import numpy as np

F = np.float32
MISS_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def valid_rays(o, d):
    """A ray whose direction is zero or not finite, or whose origin is not finite, misses everything."""
    o, d = _f(o), _f(d)
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def shear(d):
    """kx, ky, kz [N] and Sx, Sy, Sz [N] float32 of directions d [N,3] (valid rays only)."""
    d = _f(d)
    kz = np.argmax(np.abs(d), axis=1)  # the first maximum: ties go to the lowest axis
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    rows = np.arange(len(d))
    dz = d[rows, kz]
    swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, F(1.0) / dz
    return kx, ky, kz, Sx.astype(F), Sy.astype(F), Sz.astype(F)


def intersect(o, d, v0, v1, v2):
    """Every ray [N] against every triangle [T]: (hit bool [N,T], t float32 [N,T]; t is meaningless where hit is False)."""
    o, d, v0, v1, v2 = _f(o), _f(d), _f(v0), _f(v1), _f(v2)
    N = len(o)
    ok = valid_rays(o, d)
    d_safe = np.where(ok[:, None], d, F(1.0)).astype(F)
    o_safe = np.where(ok[:, None], o, F(0.0)).astype(F)
    kx, ky, kz, Sx, Sy, Sz = shear(d_safe)
    rows = np.arange(N)
    okx, oky, okz = o_safe[rows, kx][:, None], o_safe[rows, ky][:, None], o_safe[rows, kz][:, None]
    Sx, Sy, Sz = Sx[:, None], Sy[:, None], Sz[:, None]
    with np.errstate(all="ignore"):
        def sheared(v):
            vt = v.T  # [3, T]
            Pkx, Pky, Pkz = vt[kx] - okx, vt[ky] - oky, vt[kz] - okz  # [N, T]
            return Pkx - Sx * Pkz, Pky - Sy * Pkz, Pkz
        Ax, Ay, Akz = sheared(v0)
        Bx, By, Bkz = sheared(v1)
        Cx, Cy, Ckz = sheared(v2)
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        z = (U == 0) | (V == 0) | (W == 0)
        if z.any():
            D = np.float64
            e = lambda a, b, c, dd: (a[z].astype(D) * b[z].astype(D) - c[z].astype(D) * dd[z].astype(D)).astype(F)
            U[z], V[z], W[z] = e(Cx, By, Cy, Bx), e(Ax, Cy, Ay, Cx), e(Bx, Ay, By, Ax)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        Az, Bz, Cz = Sz * Akz, Sz * Bkz, Sz * Ckz
        t = ((U * Az + V * Bz) + W * Cz) / det
        hit = ~mixed & (det != 0) & (t >= 0) & np.isfinite(t) & ok[:, None]
    t = np.where(t == 0, F(0.0), t).astype(F)  # -0 -> +0
    return hit, t


def normals_of(vertices, triangles):
    """Unit cross(v1 - v0, v2 - v0) per triangle in the stated order; zeros where the length is 0 or not finite."""
    v = _f(vertices)
    a, b, c = (v[np.asarray(triangles)[:, k]] for k in range(3))
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F)
        good = (ln > 0) & np.isfinite(ln)
        out = np.where(good[:, None], n / np.where(good, ln, F(1.0))[:, None], F(0.0)).astype(F)
    return out


def cast_rays(vertices, triangles, rays_o, rays_d, chunk=256):
    """The all-triangles answer: dict(t_hit f32 [N] (inf), primitive_ids i32 [N] (-1), primitive_normals f32 [N,3],
    incidences f32 [N])."""
    v, tri = _f(vertices), np.asarray(triangles, np.int64)
    o, d = _f(rays_o), _f(rays_d)
    v0, v1, v2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    N, T = len(o), len(tri)
    keys = np.full(N, MISS_KEY, np.uint64)
    index = np.arange(T, dtype=np.uint64)[None, :]
    for s in range(0, N, chunk):
        hit, t = intersect(o[s:s + chunk], d[s:s + chunk], v0, v1, v2)
        key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index
        keys[s:s + chunk] = np.where(hit, key, MISS_KEY).min(axis=1)
    miss = keys == MISS_KEY
    ids = np.where(miss, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    t_hit = np.where(miss, np.uint32(0x7F800000), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(F)
    tn = normals_of(v, tri)
    normals = np.where(miss[:, None], F(0.0), tn[np.maximum(ids, 0)]).astype(F)
    with np.errstate(all="ignore"):
        inc = np.abs((d[:, 0] * normals[:, 0] + d[:, 1] * normals[:, 1]) + d[:, 2] * normals[:, 2]).astype(F)
    inc = np.where(miss | ~(np.abs(normals).sum(1) > 0), F(0.0), inc).astype(F)
    return {"t_hit": t_hit, "primitive_ids": ids, "primitive_normals": normals, "incidences": inc}


def moller_trumbore_hits(vertices, triangles, rays_o, rays_d, chunk=256):
    """hit bool [N] of the plain float32 Moeller-Trumbore test (two-sided, closed edges: u >= 0, v >= 0, u + v <= 1, t >= 0) —
    only to show what the contract is NOT."""
    v, tri = _f(vertices), np.asarray(triangles, np.int64)
    o, d = _f(rays_o), _f(rays_d)
    v0 = v[tri[:, 0]]
    e1, e2 = v[tri[:, 1]] - v0, v[tri[:, 2]] - v0
    out = np.zeros(len(o), bool)
    with np.errstate(all="ignore"):
        for s in range(0, len(o), chunk):
            oo, dd = o[s:s + chunk, None, :], d[s:s + chunk, None, :]
            p = np.cross(dd, e2[None])
            det = (e1[None] * p).sum(-1)
            inv = F(1.0) / det
            tv = oo - v0[None]
            u = (tv * p).sum(-1) * inv
            q = np.cross(tv, e1[None])
            w = (dd * q).sum(-1) * inv
            t = (e2[None] * q).sum(-1) * inv
            out[s:s + chunk] = ((det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= 0) & np.isfinite(t)).any(1)
    return out


# ------------------------------------------------------------------------------------------------------------- ray sets
def mesh_edges(triangles):
    t = np.asarray(triangles, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)


def rays_at_features(vertices, triangles, origin):
    """From `origin` at every vertex, every edge midpoint, every centroid, and along the six axes: (o [N,3], d [N,3]) float32,
    directions not normalised (target - origin in float32)."""
    v, t = _f(vertices), np.asarray(triangles, np.int64)
    e = mesh_edges(t)
    mid = ((v[e[:, 0]] + v[e[:, 1]]) * F(0.5)).astype(F)
    cen = ((v[t[:, 0]] + v[t[:, 1]] + v[t[:, 2]]) / F(3.0)).astype(F)
    origin = _f(origin)
    d = np.concatenate([v - origin, mid - origin, cen - origin, AXES]).astype(F)
    return np.broadcast_to(origin, d.shape).copy(), d


def grid_planes(lo, hi, n):
    """lo, cell width and the planes lo + k * w of the kernel's grid (rc_grid): extent floored at 2^-10 of the largest one."""
    lo, hi = _f(lo), _f(hi)
    ext = hi - lo
    emax = ext.max() if ext.max() > 0 else F(1.0)
    e = np.maximum(ext, emax * F(2.0 ** -10)).astype(F)
    w = (e / np.asarray(n, F)).astype(F)
    return lo, w, [(lo[a] + np.arange(n[a] + 1, dtype=F) * w[a]).astype(F) for a in range(3)]
