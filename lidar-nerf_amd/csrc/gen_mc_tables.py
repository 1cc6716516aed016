#!/usr/bin/env python3
"""Generates csrc/mc_tables.h: the 256 marching-cubes cases of csrc/mesh.hip, derived by program (no table is copied from
anywhere; triangle order and the choice on ambiguous cases are this file's own, not PyMCubes').

Numbering.  Corner i of a cell sits at offset (i & 1, i >> 1 & 1, i >> 2 & 1) = (dx, dy, dz); bit i of the case is set iff
that corner is BELOW (v < iso).  Edge e = 4 * axis + k runs along `axis` (0 x, 1 y, 2 z) from its lower corner, whose two
other offsets are (k & 1, k >> 1) in increasing axis order: x edges (dy, dz), y edges (dx, dz), z edges (dx, dy).  The
lower corner of an edge is the lattice point that owns its vertex.

Rules.  An edge crosses iff exactly one end is below.  On each of the six faces the four corner bits alone give the segments
between crossing edges: one below (or one not-below) corner is cut off by one segment; two neighbouring below corners by
one segment between the two other edges; two DIAGONAL below corners by two segments, each cutting off one below corner.
Two cells that share a face read the same four bits, so they agree.  Every segment is directed so that, seen from outside
the cell, the below side lies to its left; the segments then chain into closed directed loops, taken in the order of their
lowest-numbered edge.  Each loop is fan-triangulated from its lowest-numbered edge whose fan keeps every diagonal off the
cell's faces (fan()).  With normal = (b - a) x (c - a) the triangles' normals point to the below side: on a density field,
out of the dense matter (a closed surface around dense matter has positive signed volume).

Run:  python lidar-nerf_amd/csrc/gen_mc_tables.py > lidar-nerf_amd/csrc/mc_tables.h"""

CORNERS = [(i & 1, i >> 1 & 1, i >> 2 & 1) for i in range(8)]


def edge_ends(e):
    """(lower corner, upper corner) of edge e."""
    axis, k = divmod(e, 4)
    off = [0, 0, 0]
    others = [a for a in range(3) if a != axis]
    off[others[0]], off[others[1]] = k & 1, k >> 1
    lo = off[0] | off[1] << 1 | off[2] << 2
    return lo, lo | 1 << axis


EDGES = [edge_ends(e) for e in range(12)]
EDGE_OF = {ends: e for e, ends in enumerate(EDGES)}


def edge_between(c0, c1):
    return EDGE_OF[(min(c0, c1), max(c0, c1))]


def faces():
    """Six faces as (outward normal, the four corners in cyclic order)."""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            ring = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[u], off[v] = side, cu, cv
                ring.append(off[0] | off[1] << 1 | off[2] << 2)
            normal = [0, 0, 0]
            normal[axis] = 1 if side else -1
            out.append((tuple(normal), ring))
    return out


FACES = faces()


def _mid2(e):
    """Twice the midpoint of edge e (integers)."""
    a, b = (CORNERS[c] for c in EDGES[e])
    return tuple(p + q for p, q in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _directed(ea, eb, corner, corner_is_below, normal):
    """The segment between edges ea and eb that cuts `corner` off, directed with the below side on its left seen from
    outside (along -normal)."""
    A, B = _mid2(ea), _mid2(eb)
    C = tuple(2 * p for p in CORNERS[corner])
    ab = tuple(q - p for p, q in zip(A, B))
    ac = tuple(q - p for p, q in zip(A, C))
    left = sum(x * n for x, n in zip(_cross(ab, ac), normal)) > 0  # `corner` lies to the left of A -> B
    return (ea, eb) if left == corner_is_below else (eb, ea)


def face_segments(case, face):
    """Directed segments (edge, edge) the face rule prescribes on `face` = (normal, ring) for this case."""
    normal, ring = face
    below = [bool(case >> c & 1) for c in ring]
    n = sum(below)
    if n in (0, 4):
        return []

    def cut(i):  # the segment around ring corner i
        return _directed(edge_between(ring[i], ring[i - 1]), edge_between(ring[i], ring[(i + 1) % 4]), ring[i], below[i],
                         normal)

    if n == 1:
        return [cut(below.index(True))]
    if n == 3:
        return [cut(below.index(False))]
    if below[0] == below[2]:  # two diagonal corners below: each is cut off on its own
        return [cut(i) for i in range(4) if below[i]]
    i = next(i for i in range(4) if below[i] and below[(i + 1) % 4])  # two neighbours below
    j = (i + 1) % 4
    return [_directed(edge_between(ring[i], ring[i - 1]), edge_between(ring[j], ring[(j + 1) % 4]), ring[i], True, normal)]


def crossing_edges(case):
    return [e for e, (a, b) in enumerate(EDGES) if (case >> a & 1) != (case >> b & 1)]


def case_loops(case):
    nxt = {}
    for face in FACES:
        for a, b in face_segments(case, face):
            assert a not in nxt
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()) == crossing_edges(case)
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        loops.append(loop)
    return loops


EDGE_FACES = [{f for f, (_, ring) in enumerate(FACES) if set(EDGES[e]) <= set(ring)} for e in range(12)]


def fan(loop):
    """The loop rotated to the apex of its fan: its lowest-numbered edge from which no diagonal of the fan lies inside a cube
    face.  (A loop that passes an ambiguous face twice has two edges on that face that are not neighbours in the loop; a
    diagonal between them would lie IN the face, where the cell behind it may put one too: an edge with four triangles.  18
    loops of the 256 cases move their apex for this; every loop has such an apex.)"""
    n = len(loop)
    for apex in sorted(loop):
        s = loop.index(apex)
        rot = loop[s:] + loop[:s]
        if all(not (EDGE_FACES[rot[0]] & EDGE_FACES[rot[i]]) for i in range(2, n - 1)):
            return rot
    raise AssertionError(f"no fan of {loop} stays off the faces")


def case_triangles(case):
    """Triangles of a case as triples of edge numbers."""
    return [(rot[0], rot[i], rot[i + 1]) for rot in map(fan, case_loops(case)) for i in range(1, len(rot) - 1)]


TRIANGLES = [case_triangles(c) for c in range(256)]
TRI_COUNT = [len(t) for t in TRIANGLES]
MAX_TRIANGLES = max(TRI_COUNT)


def header():
    pad = 3 * MAX_TRIANGLES
    lines = ["// GENERATED by gen_mc_tables.py — do not edit.  Numbering, face rule and winding: see the generator.",
             "// kMcTriCount[case]: triangles of the case; kMcTriEdges[case]: their corners as edge numbers (4 * axis + k), -1 padded.",
             "#pragma once",
             f"constexpr int kMcMaxTriangles = {MAX_TRIANGLES};",
             "__device__ constexpr unsigned char kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(n) for n in TRI_COUNT[r:r + 32]) + ",")
    lines += ["};", f"__device__ constexpr signed char kMcTriEdges[256][{pad}] = {{"]
    for c in range(256):
        flat = [e for t in TRIANGLES[c] for e in t]
        flat += [-1] * (pad - len(flat))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    print(header(), end="")
