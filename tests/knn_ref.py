"""NumPy restatement of the k-nearest-neighbour contract of csrc/knn.hip (include/lidarnerf_hip.h, lnh_knn_*): float32 operations
in the stated order, nothing shared with the library.

Two parts.  brute_force: the keys (bits of d2) << 32 | index over ALL points, sorted — the contract.  grid_walk: the shells of
cells around the query's cell with the stopping rule of DESIGN §16 — the argument that a grid never changes the answer, restated
so that it can be compared with the brute force without a GPU."""
import numpy as np

F = np.float32
INF = np.float32(np.inf)
EMPTY = np.uint64(0xffffffffffffffff)


def dist2(points, q):
    """d2 = ((dx dx) + (dy dy)) + (dz dz), every operation one float32 operation.  points [N,3] f32, q [3] f32 -> [N] f32."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = points[:, 0] - q[0], points[:, 1] - q[1], points[:, 2] - q[2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def keys_of(points, q, index=None):
    d2 = dist2(points, q)
    assert d2.dtype == np.float32
    index = np.arange(len(points), dtype=np.uint64) if index is None else index.astype(np.uint64)
    return d2.view(np.uint32).astype(np.uint64) << np.uint64(32) | index


def _unpack(keys, k):
    """Sorted keys (at most k) -> (indices i32 [k], dist2 f32 [k]) with -1 / +inf behind them."""
    idx, d2 = np.full(k, -1, np.int32), np.full(k, INF, np.float32)
    n = len(keys)
    idx[:n] = (keys & np.uint64(0xffffffff)).astype(np.int32)
    d2[:n] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2


def brute_force(points, queries, k, valid=None, chunk=2048):
    """(indices i32 [Q,k], dist2 f32 [Q,k]): the min(k, N) smallest keys over all points, ascending; -1 / +inf behind them, for
    a query with valid == 0 and for a query with a non-finite coordinate.  (Blocks of queries at a time: the same float32
    operations, element by element.)"""
    points, queries = np.ascontiguousarray(points, F), np.ascontiguousarray(queries, F)
    Q, N = len(queries), len(points)
    idx, d2 = np.full((Q, k), -1, np.int32), np.full((Q, k), INF, np.float32)
    live = np.isfinite(queries).all(1) & (np.ones(Q, bool) if valid is None else np.asarray(valid).astype(bool))
    index = np.arange(N, dtype=np.uint64)
    held = min(k, N)
    for first in range(0, Q, chunk):
        q = queries[first:first + chunk]
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy, dz = (points[None, :, a] - q[:, None, a] for a in range(3))
            dd = ((dx * dx) + (dy * dy)) + (dz * dz)
        assert dd.dtype == np.float32
        keys = dd.view(np.uint32).astype(np.uint64) << np.uint64(32) | index
        if N > k:
            keys = np.partition(keys, k - 1, axis=1)[:, :k]
        keys = np.sort(keys, axis=1)
        idx[first:first + chunk, :held] = (keys & np.uint64(0xffffffff)).astype(np.int32)
        d2[first:first + chunk, :held] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    idx[~live], d2[~live] = -1, INF
    return idx, d2


def mean_of(values, indices):
    """f32 [Q]: the neighbours' values summed in rank order in float64, divided by their number, rounded once; 0 without any."""
    values, indices = np.ascontiguousarray(values, F), np.asarray(indices)
    s, n = np.zeros(len(indices), np.float64), np.zeros(len(indices), np.float64)
    for j in range(indices.shape[1]):  # rank by rank: the order of the sum
        has = indices[:, j] >= 0
        s = np.where(has, s + values[np.maximum(indices[:, j], 0)].astype(np.float64), s)
        n = n + has
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, 0.0).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- the grid
class Grid:
    """The build: box, cell function, the cell of every point, the slab extremes smin / pmax."""

    def __init__(self, points, grid):
        p = self.points = np.ascontiguousarray(points, F)
        self.n = tuple(int(x) for x in grid)
        self.lo, self.hi = p.min(0), p.max(0)
        ext = self.hi - self.lo
        emax = ext.max()
        if not emax > 0 or not np.isfinite(emax):
            emax = F(1.0)
        e = np.maximum(ext, emax * F(0.0009765625))
        self.inv = np.array(self.n, F) / e
        assert self.inv.dtype == np.float32
        self.cells = np.stack([self.cell_of(p[:, a], a) for a in range(3)], 1)
        self.smin, self.pmax = [], []
        for a in range(3):
            lo, hi = np.full(self.n[a], INF, F), np.full(self.n[a], -INF, F)
            np.minimum.at(lo, self.cells[:, a], p[:, a])
            np.maximum.at(hi, self.cells[:, a], p[:, a])
            self.smin.append(np.minimum.accumulate(lo[::-1])[::-1])  # over the slabs >= i
            self.pmax.append(np.maximum.accumulate(hi))              # over the slabs <= i

    def cell_of(self, x, a):
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.floor((np.asarray(x, F) - self.lo[a]) * self.inv[a])
        return np.minimum(np.maximum(c, F(0.0)), F(self.n[a] - 1)).astype(np.int64)


def grid_walk(g, queries, k, stats=None):
    """The same answer as brute_force(g.points, queries, k), found shell by shell with the stopping rule."""
    queries = np.ascontiguousarray(queries, F)
    Q = len(queries)
    idx, d2 = np.full((Q, k), -1, np.int32), np.full((Q, k), INF, np.float32)
    every = np.arange(len(g.points))
    for i in range(Q):
        q = queries[i]
        if not np.isfinite(q).all():
            continue
        c = [int(g.cell_of(q[a], a)) for a in range(3)]
        ring = np.abs(g.cells - np.array(c)).max(1)  # the shell of every point
        held = np.empty(0, np.uint64)
        r = 0
        while True:
            member = every[ring == r]
            if len(member):  # every point of the shell, before the stopping test is looked at
                held = np.sort(np.concatenate([held, keys_of(g.points[member], q, member)]))[:k]
            gaps = []
            with np.errstate(over="ignore"):
                for a in range(3):
                    if c[a] + r + 1 <= g.n[a] - 1:
                        gaps.append(np.maximum(g.smin[a][c[a] + r + 1] - q[a], F(0.0)))
                    if c[a] - r - 1 >= 0:
                        gaps.append(np.maximum(q[a] - g.pmax[a][c[a] - r - 1], F(0.0)))
                if not gaps:  # the block covers the grid
                    break
                gmin = np.min(np.array(gaps, F))
                bound = gmin * gmin
            assert bound.dtype == np.float32
            if len(held) == k and (held[k - 1] >> np.uint64(32)).astype(np.uint32).view(np.float32) < bound:
                break
            r += 1
        if stats is not None:
            stats.append((r, int((ring <= r).sum())))
        idx[i], d2[i] = _unpack(held, k)
    return idx, d2


# ------------------------------------------------------------------------------------------------------------- the clouds
def clouds(n=3000, seed=5):
    """The six clouds of the tests, at most n points each: uniform, a lattice full of ties, duplicated points, a flat cloud, a
    far-away cluster and a single point."""
    rng = np.random.default_rng(seed)
    uniform = rng.uniform([-3, 0, 100], [7, 4, 107], (n, 3)).astype(F)
    side = max(2, int(round(n ** (1 / 3))) - 1)
    lattice = np.stack(np.meshgrid(*[np.arange(side, dtype=F)] * 3, indexing="ij"), -1).reshape(-1, 3) * F(0.5)
    lattice = lattice[rng.permutation(len(lattice))][:n]
    dup = np.concatenate([uniform[:n // 2], uniform[:n - n // 2]])[rng.permutation(n)]
    flat = uniform.copy()
    flat[:, 2] = F(2.5)
    far = uniform.copy()
    far[::7] += np.array([500, -300, 0], F)
    return {"uniform": uniform, "lattice": np.ascontiguousarray(lattice), "duplicates": np.ascontiguousarray(dup), "flat": flat,
            "far_cluster": far, "one_point": uniform[:1].copy()}


def queries_for(points, n, seed=11):
    """n queries: on points, within 1e-3 of points, inside the box, far outside it (a quarter each, mixed)."""
    rng = np.random.default_rng(seed + len(points))
    lo, hi = points.min(0), points.max(0)
    ext = np.maximum(hi - lo, F(1.0))
    m = (n + 3) // 4
    on = points[rng.integers(0, len(points), m)]
    near = points[rng.integers(0, len(points), m)] + rng.uniform(-1e-3, 1e-3, (m, 3)).astype(F)
    inside = rng.uniform(lo, hi, (m, 3))
    outside = lo - 3 * ext + rng.uniform(0, 1, (m, 3)) * 7 * ext
    q = np.concatenate([on, near, inside, outside]).astype(F)
    return np.ascontiguousarray(q[rng.permutation(len(q))][:n])
