"""NumPy restatement of the four contracts of csrc/tsdf.hip (include/lidarnerf_hip.h: lnh_tsdf_integrate, lnh_tsdf_finalize,
lnh_mesh_vertex_observed, lnh_mesh_filter_*), operation by operation: float32 arithmetic in the header's order, atan2 in float64
rounded to float32, the frames in order.  Vectorised over the lattice, one frame at a time.  Plus what the tests share: the
lattice rule of lidarnerf.tsdf.TSDFVolume, the hand-chained extract_mesh over tests/marching_cubes_ref.py, and the two closed-form
scenes (a sphere of constant depth, a box room) with their range images."""
import functools

import numpy as np

import marching_cubes_ref as mc

F = np.float32
FILL = F(1.0)
PI = 3.14159265358979323846


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------ geometry
def pano_geom(H, W, fov_up, fov):
    """(pi_f, down_rad, col_step, row_step) as csrc/pano_geom.h forms them on the host: in double from the float32 arguments,
    rounded to float32 once."""
    fov_up, fov = float(F(fov_up)), float(F(fov))
    return F(PI), F((fov - fov_up) / 180.0 * PI), F(2.0 * PI / float(W)), F(fov / 180.0 * PI / float(H))


def atan2_rn(y, x):
    return np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F)


def project(qx, qy, qz, H, W, fov_up, fov, max_depth, wrap=True):
    """(ok bool, row-major pixel int64 (0 where not ok), r float32) of points in the sensor frame: pano_pixel_xyz of
    csrc/pano_geom.h.  wrap=False is lnh_lidar_to_pano's own rule (a column that rounds to W is dropped)."""
    pi_f, down_rad, col_step, row_step = pano_geom(H, W, fov_up, fov)
    with np.errstate(all="ignore"):
        r = np.sqrt((qx * qx + qy * qy) + qz * qz)
        ok = (r < F(max_depth)) & (r > F(0))
        beta = pi_f - atan2_rn(qy, qx)
        alpha = atan2_rn(qz, np.sqrt(qx * qx + qy * qy)) + down_rad
        cf = np.rint(beta / col_step)
        rf = np.rint(F(H) - alpha / row_step)
        if wrap:
            cf = np.where(cf == F(W), F(0), cf)
        ok = ok & (rf >= 0) & (cf >= 0) & (rf < F(H)) & (cf < F(W))
        pix = np.where(ok, rf, F(0)).astype(np.int64) * W + np.where(ok, cf, F(0)).astype(np.int64)
    return ok, pix, r


def lattice_axes(lo, step, dims):
    """p_a = lo[a] + float(i) * step[a] as broadcastable float32 arrays [nx,1,1], [1,ny,1], [1,1,nz]."""
    lo, step = _f(lo), _f(step)
    shape = ([-1, 1, 1], [1, -1, 1], [1, 1, -1])
    return [(lo[a] + np.arange(dims[a], dtype=F) * step[a]).astype(F).reshape(shape[a]) for a in range(3)]


# ------------------------------------------------------------------------------------------------------- the contracts
def integrate(panos, world_to_lidar, fov_up, fov, max_depth, lo, step, dims, trunc, sum_, count, wrap=True):
    """lnh_tsdf_integrate: returns the new (sum float32 [nx,ny,nz], count uint32 [nx,ny,nz]); the inputs are left alone."""
    panos, m_all = _f(panos), _f(world_to_lidar).reshape(-1, 12)
    n_frames, H, W = panos.shape
    assert len(m_all) == n_frames
    px, py, pz = lattice_axes(lo, step, dims)
    s = _f(sum_).reshape(dims).copy()
    c = np.ascontiguousarray(count, np.uint32).reshape(dims).copy()
    trunc = F(trunc)
    for f in range(n_frames):
        m = m_all[f]
        qx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
        qy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
        qz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
        ok, pix, r = project(qx, qy, qz, H, W, fov_up, fov, max_depth, wrap)
        with np.errstate(all="ignore"):
            d = panos[f].reshape(-1)[pix]
            ok = ok & (d > 0) & (d < np.inf)
            sd = d - r
            ok = ok & ~(sd < -trunc)
            s = np.where(ok, s + np.minimum(sd / trunc, F(1)), s).astype(F)
        c = c + ok.astype(np.uint32)
    return s, c


def finalize(sum_, count, min_count=1):
    """lnh_tsdf_finalize: -(sum / float(count)) where count >= min_count, else the fill."""
    assert min_count >= 1
    with np.errstate(all="ignore"):
        v = -(_f(sum_) / np.asarray(count).astype(F))
    return np.where(np.asarray(count) >= min_count, v, FILL).astype(F)


def vertex_observed(vertices, count, min_count=1):
    """lnh_mesh_vertex_observed: uint8 [V]."""
    v = _f(vertices).reshape(-1, 3)
    count = np.asarray(count)
    dims = count.shape
    hi = np.asarray(dims, F) - F(1)
    with np.errstate(invalid="ignore"):
        inside = ((v >= 0) & (v <= hi)).all(1)  # (dims <= 2^24 here; the kernel compares in integers behind the floor)
    safe = np.where(inside[:, None], v, F(0))
    fl = np.floor(safe)
    far = (safe != fl).astype(np.int64)
    base = fl.astype(np.int64)
    seen = inside.copy()
    for k in range(8):
        q = base + far * np.array([k & 1, k >> 1 & 1, k >> 2])
        seen &= count[q[:, 0], q[:, 1], q[:, 2]] >= min_count
    return seen.astype(np.uint8)


def mesh_filter(vertices, keep, triangles):
    """lnh_mesh_filter_*: (kept vertices in order, triangles with three kept in-range corners in order, renumbered)."""
    v, keep = _f(vertices).reshape(-1, 3), np.asarray(keep).astype(bool)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    in_range = ((t >= 0) & (t < len(v))).all(1)
    stays = in_range & keep[np.where(in_range[:, None], t, 0)].all(1)
    new_index = np.cumsum(keep) - keep
    return v[keep], new_index[t[stays]].astype(np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------- the Python layer's rules
def lattice_of(box_min, box_max, resolution=None, voxel_size=None):
    """(lo float32 [3], step float32 [3], dims) of lidarnerf.tsdf.TSDFVolume: `resolution` points per axis from end to end of
    the box, or points `voxel_size` apart from its minimum, ceil(extent / voxel_size) of them per axis."""
    lo, hi = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    if voxel_size is None:
        dims = (int(resolution),) * 3
        step = (hi - lo) / (int(resolution) - 1)
    else:
        dims = tuple(max(2, int(np.ceil(e / float(voxel_size) - 1e-6))) for e in (hi - lo))
        step = np.full(3, float(voxel_size))
    return lo.astype(F), step.astype(F), dims


def to_world(vertices, lo, step):
    """Index units -> world: lo + v * step in float64 on the float32 lattice numbers, rounded to float32 once."""
    return (_f(lo).astype(np.float64)[None, :] + _f(vertices).astype(np.float64) * _f(step).astype(np.float64)[None, :]).astype(F)


def extract_mesh(sum_, count, lo, step, min_count=1):
    """The chain of TSDFVolume.extract_mesh by hand: finalize, marching cubes at 0, vertex mask, filter, world units.  Also
    returns the intermediate arrays."""
    vol = finalize(sum_, count, min_count)
    v, t, _ = mc.marching_cubes(vol, 0.0)
    keep = vertex_observed(v, count, min_count)
    fv, ft = mesh_filter(v, keep, t)
    return to_world(fv, lo, step), ft, dict(volume=vol, vertices=v, triangles=t, keep=keep, kept_vertices=fv)


# --------------------------------------------------------------------------------------------------------------- scenes
def pixel_directions(H, W, fov_up, fov):
    """Unit directions [H,W,3] float64 of the pixel centres (pano_to_lidar's angles)."""
    i = np.arange(W, dtype=np.float64)[None, :]
    j = np.arange(H, dtype=np.float64)[:, None]
    beta = -(i - W / 2) / W * 2 * np.pi
    alpha = (fov_up - j / H * fov) / 180 * np.pi
    return np.stack([np.cos(alpha) * np.cos(beta), np.cos(alpha) * np.sin(beta), np.sin(alpha) + 0 * beta], -1)


def translation_pose(t):
    pose = np.eye(4, dtype=F)
    pose[:3, 3] = t
    return pose


def inverse_affine(pose):
    """world -> lidar [12] float32 of a lidar -> world pose, by cofactors in float32 (lidarnerf.nvs.inverse_pose's operations)."""
    A, t = _f(pose)[:3, :3], _f(pose)[:3, 3]
    c0, c1, c2 = np.cross(A[:, 1], A[:, 2]).astype(F), np.cross(A[:, 2], A[:, 0]).astype(F), np.cross(A[:, 0], A[:, 1]).astype(F)
    det = (A[:, 0] * c0).sum(dtype=F)
    inv = (np.stack([c0, c1, c2]) / det).astype(F)
    back = -((inv[:, 0] * t[0] + inv[:, 1] * t[1]) + inv[:, 2] * t[2])
    return np.concatenate([inv, back[:, None]], 1).astype(F).reshape(12)


ROOM_LO, ROOM_HI = np.array([-6.0, -4.0, -1.7]), np.array([6.0, 4.0, 3.0])
ROOM_K, ROOM_HW, ROOM_H = (2.0, 26.9), (66, 1030), 0.2
ROOM_SENSORS = tuple((x, 0.3 * x, 0.0) for x in (-1.5, -0.5, 0.5, 1.5))


def room_depths(origin, H, W, fov_up, fov):
    """The range image of the box room seen from `origin` (inside it), in closed form: float32 [H,W]."""
    d = pixel_directions(H, W, fov_up, fov)
    o = np.asarray(origin, np.float64)
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, (ROOM_HI - o) / d, np.where(d < 0, (ROOM_LO - o) / d, np.inf))
    return t.min(-1).astype(F)


@functools.lru_cache(maxsize=None)
def room(drop=0.0, seed=7):
    """The closed-loop scene of the issue: four frames of 66 x 1030 from ROOM_SENSORS, no rotation; the lattice h = 0.2 over the room
    plus 0.55 (66 x 46 x 29), trunc = 3 h; fused with the restatement.  drop: the share of pixels set to 0 (seeded).  Read-only."""
    H, W = ROOM_HW
    panos = np.stack([room_depths(s, H, W, *ROOM_K) for s in ROOM_SENSORS])
    if drop:
        panos = np.where(np.random.default_rng(seed).random(panos.shape) < drop, F(0), panos).astype(F)
    poses = np.stack([translation_pose(s) for s in ROOM_SENSORS])
    w2l = np.stack([inverse_affine(p) for p in poses])
    lo, step, dims = lattice_of(ROOM_LO - 0.55, ROOM_HI + 0.55, voxel_size=ROOM_H)
    assert dims == (66, 46, 29)
    trunc = F(3) * step.max()
    s, c = integrate(panos, w2l, *ROOM_K, 80.0, lo, step, dims, trunc, np.zeros(dims, F), np.zeros(dims, np.uint32))
    out = dict(panos=panos, poses=poses, w2l=w2l, lo=lo, step=step, dims=dims, trunc=trunc, sum=s, count=c)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def room_mesh(drop=0.0):
    r = room(drop)
    v, t, parts = extract_mesh(r["sum"], r["count"], r["lo"], r["step"])
    for a in (v, t, *parts.values()):
        a.setflags(write=False)
    return v, t, parts


def closed_loop(cast, frame, n_rays=600, seed=11, drop=0.0):
    """Rays through `n_rays` seeded pixels of training frame `frame` that hold a depth, cast back by cast(o [N,3], d [N,3]) ->
    (t_hit [N] (inf on a miss), normals [N,3]): (hit share, |t - depth| of the hits in units of h, every hit normal faces the
    sensor)."""
    pick, o, d, depth = closed_loop_rays(frame, n_rays, seed, drop)
    t_hit, normals = cast(o, d)
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    return closed_loop_figures(np.asarray(t_hit, np.float64) * length, normals, d, depth)


def closed_loop_rays(frame, n_rays=600, seed=11, drop=0.0):
    """(pixel ids [N], origins [N,3], directions [N,3] float32, depths [N]) of the seeded pixels of training frame `frame`."""
    H, W = ROOM_HW
    depth = room(drop)["panos"][frame].reshape(-1)
    pick = np.random.default_rng(seed + frame).choice(np.flatnonzero(depth > 0), n_rays, replace=False)
    d = pixel_directions(H, W, *ROOM_K).reshape(-1, 3)[pick].astype(F)
    return pick, np.broadcast_to(np.asarray(ROOM_SENSORS[frame], F), d.shape).copy(), d, depth[pick]


def closed_loop_figures(found, normals, d, depth):
    """found [N]: the depth a ray came back with (inf on a miss) -> (hit share, |found - depth| / h of the hits, every hit normal
    faces the sensor)."""
    hit = np.isfinite(found)
    err = np.abs(np.asarray(found, np.float64)[hit] - depth[hit]) / ROOM_H
    facing = np.einsum("ij,ij->i", np.asarray(normals, np.float64)[hit], d[hit].astype(np.float64)) < 0
    return float(hit.mean()), err, bool(facing.all())


SPHERE = dict(d0=4.0, h=0.25, K=(2.0, 26.9), HW=(66, 1030), box=(-5.0, 5.25))


@functools.lru_cache(maxsize=None)
def sphere():
    """One frame of constant depth d0 with an identity pose: the volume is a function of r alone.  Lattice h = 0.25 over
    [-5, 5]^3 (41^3 points; every coordinate a multiple of 0.25, exact in float32), trunc = 3 h."""
    H, W = SPHERE["HW"]
    lo, step, dims = lattice_of([SPHERE["box"][0]] * 3, [SPHERE["box"][1]] * 3, voxel_size=SPHERE["h"])
    assert dims == (41, 41, 41)  # -5 ... 5
    panos = np.full((1, H, W), SPHERE["d0"], F)
    w2l = inverse_affine(np.eye(4, dtype=F))[None]
    trunc = F(3) * step.max()
    s, c = integrate(panos, w2l, *SPHERE["K"], 80.0, lo, step, dims, trunc, np.zeros(dims, F), np.zeros(dims, np.uint32))
    out = dict(panos=panos, w2l=w2l, lo=lo, step=step, dims=dims, trunc=trunc, sum=s, count=c)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def sphere_rounding_term():
    """The rounding part of the sphere bound (derived in tests/test_tsdf_cpu.py::test_sphere_vertices_lie_on_the_sphere)."""
    h, trunc = SPHERE["h"], 3 * SPHERE["h"]
    return 2.0 ** -22 + trunc * 2.0 ** -24 + h * 2.0 ** -23 + h * 2.0 ** -19 + 2.0 ** -22


def check_sphere_vertices(world_vertices):
    """(largest |r(v) - d0|, its bound, largest excess of a vertex's elevation over the image's band in pixels of elevation, the
    allowed excess) for the sphere scene."""
    d0, h, (fov_up, fov), (H, W) = SPHERE["d0"], SPHERE["h"], SPHERE["K"], SPHERE["HW"]
    v = np.asarray(world_vertices, np.float64)
    r = np.linalg.norm(v, axis=1)
    bound = h * h / (8 * (d0 - h)) + sphere_rounding_term()
    elev = np.degrees(np.arctan2(v[:, 2], np.hypot(v[:, 0], v[:, 1])))
    pixel = fov / H
    excess = np.maximum(elev - fov_up, (fov_up - fov) - elev) / pixel
    return float(np.abs(r - d0).max()), bound, float(excess.max()), 0.5
