// raycast.hip — closest-hit ray casting against a triangle mesh on the GPU: what lidarnvs/lidarnvs_meshing.py does with
// Open3D's RaycastingScene.cast_rays (Embree on the host) in intersect_rays / intersect_lidar / predict_frame_with_raydrop.
//
// THE INTERSECTION FUNCTION (rc_intersect; Woop, Benthin, Wald: "Watertight Ray/Triangle Intersection", JCGT 2013), fp32, the
// library is built with -ffp-contract=off, every line below is one rounded operation per operator, in this order:
//   kz = axis of the largest |d| (ties: the lowest axis); kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped when d[kz] < 0
//   Sx = d[kx] / d[kz]      Sy = d[ky] / d[kz]      Sz = 1 / d[kz]
//   per vertex P in (A, B, C) = (v0, v1, v2):  Pkx = P[kx] - o[kx]   Pky = P[ky] - o[ky]   Pkz = P[kz] - o[kz]
//                                              Px = Pkx - Sx * Pkz   Py = Pky - Sy * Pkz
//   U = Cx * By - Cy * Bx      V = Ax * Cy - Ay * Cx      W = Bx * Ay - By * Ax
//   if U == 0 or V == 0 or W == 0: all three again from the same fp32 operands in double (the products are exact, the
//       difference is rounded to double), each converted to fp32
//   miss if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0)         (two-sided: no culling)
//   det = (U + V) + W;  miss if det == 0
//   Pz = Sz * Pkz;  t = ((U * Az + V * Bz) + W * Cz) / det                   (ONE division)
//   miss unless t >= 0 and t is finite; a t equal to zero is stored as +0
// t is in units of the length of d as given.  A ray whose direction is zero or not finite, or whose origin is not finite,
// misses everything.  Two triangles that share an edge compute the edge function of that edge from the same operands (a
// product of two floats commutes, a difference changes sign exactly), so a ray can never pass between them.
//
// THE ANSWER FOR A RAY is the minimum over all triangles that hit of the 64-bit key (bits of t) << 32 | triangle index: the
// nearest hit, among equal t the smallest index.  Normal of the winner: e1 = v1 - v0, e2 = v2 - v0, n = (e1y e2z - e1z e2y,
// e1z e2x - e1x e2z, e1x e2y - e1y e2x), len = sqrtf((nx nx + ny ny) + nz nz), n / len (one sqrtf, three divisions; zeros when
// len is 0 or not finite).  Incidence: |(d0 n0 + d1 n1) + d2 n2| with d as given.
//
// THE GRID only skips triangles that cannot win (DESIGN §15 has the argument).  Box = exact min / max of the vertices;
// extent e[a] = max(hi[a] - lo[a], largest extent * 2^-10) (1 when the mesh is one point), cell width w[a] = e[a] / n[a],
// cell_of(x) = clamp(floorf((x - lo[a]) * (n[a] / e[a])), 0, n[a] - 1): monotone, shared by the build and the cast.  A triangle
// is listed in every cell its bounding box, dilated by delta[a] = w[a] / 16, reaches.  The cast walks the cells of the box
// dilated by delta along the ray; the parameter at which the ray leaves a cell along axis a is (plane - o[a]) * (1 / d[a]),
// formed anew from the plane's index at every step (nothing accumulates; an axis with d[a] == 0 is never stepped and never
// multiplied).  Every triangle of a cell is tested before the key is looked at.  With tau = (largest triangle extent along kz
// + slack) / |d[kz]| — the most the computed t of a triangle can lie from where the ray really meets it — the walk begins at
// max(entry of the box, -tau) and stops when best t + tau <= the parameter at which the ray leaves the current cell.  A ray
// for which the error bound of this arithmetic, E = 2^-18 * max(|box|, |o|), is not below delta / 4 (an origin very far
// away, a mesh very far from zero, absurd magnitudes) takes the list of ALL triangles instead: the answer is the same.
//
// The grid itself (box -> cells, cell_of, the bounds passes' reduce) is cell_grid.h, shared with knn.hip; the scan is scan.h.
// Build passes, none waits for another workgroup: k_rc_bounds (per-workgroup min / max / counts, no atomics), k_rc_bounds_finish
// (one workgroup), k_rc_count (integer atomics per cell), k_rc_scan (one workgroup, scan.h workgroup_scan in 64 bits), k_rc_fill
// (an integer cursor per cell: the order inside a cell is arrival order and no output depends on it).
#include "cell_grid.h"
#include "common.h"
#include "scan.h"

namespace {

constexpr uint32_t kRcThreads = kCellThreads;
// per-workgroup partial (cell_grid.h): lo[3], hi[3], largest triangle extent[3], bad coords, bad indices, 0
constexpr uint32_t kRcBoundsWords = 12;
constexpr uint32_t kRcCastThreads = 128;
constexpr float kRcDilate = 0.0625f;                 // delta = w / 16
constexpr float kRcErrScale = 3.814697265625e-06f;   // 2^-18 = 64 ulp-fractions of fp32: E = this * magnitude
constexpr float kRcBig = 1.152921504606846976e18f, kRcSmall = 8.67361737988403547e-19f;  // 2^60, 2^-60

__device__ __forceinline__ float sel3(float a, float b, float c, uint32_t k) { return k == 0 ? a : (k == 1 ? b : c); }

// the cells (cell_grid.h) and what the cast needs besides: the box's far corner, the cell width w = e / n from the same floored
// extent e as inv = n / e, the dilation delta = w / 16, the largest triangle extent per axis
struct RcGrid : CellGrid {
    float hi[3], w[3], delta[3], maxext[3];
};
__device__ __forceinline__ RcGrid rc_grid(const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz) {
    RcGrid g;
    const uint32_t n[3] = {nx, ny, nz};
#pragma unroll
    for (int a = 0; a < 3; a++) g.hi[a] = box[3 + a], g.maxext[a] = box[6 + a];
    static_cast<CellGrid &>(g) = cell_grid(box, nx, ny, nz, [&](int a, float e) {
        g.w[a] = e / (float)n[a];
        g.delta[a] = g.w[a] * kRcDilate;
    });
    return g;
}

// ------------------------------------------------------------------------------------------------------- intersection
struct RcShear {
    uint32_t kx, ky, kz;
    float Sx, Sy, Sz;
};
__device__ __forceinline__ RcShear rc_shear(float d0, float d1, float d2) {
    RcShear s;
    const float a0 = fabsf(d0), a1 = fabsf(d1), a2 = fabsf(d2);
    s.kz = (a0 >= a1 && a0 >= a2) ? 0u : (a1 >= a2 ? 1u : 2u);
    s.kx = s.kz == 2 ? 0u : s.kz + 1;
    s.ky = s.kx == 2 ? 0u : s.kx + 1;
    const float dz = sel3(d0, d1, d2, s.kz);
    if (dz < 0.0f) {
        const uint32_t t = s.kx;
        s.kx = s.ky, s.ky = t;
    }
    s.Sx = sel3(d0, d1, d2, s.kx) / dz;
    s.Sy = sel3(d0, d1, d2, s.ky) / dz;
    s.Sz = 1.0f / dz;
    return s;
}
__device__ __forceinline__ float rc_edge_double(float a, float b, float c, float d) {
    return (float)((double)a * (double)b - (double)c * (double)d);
}
// (origin, sheared direction, v0, v1, v2) -> hit, t: the file header's function after its first two lines
__device__ __forceinline__ bool rc_intersect_sheared(const float (&o)[3], const RcShear &s, const float *__restrict__ v0,
                                                     const float *__restrict__ v1, const float *__restrict__ v2, float &t_out) {
    const float okx = sel3(o[0], o[1], o[2], s.kx), oky = sel3(o[0], o[1], o[2], s.ky), okz = sel3(o[0], o[1], o[2], s.kz);
    const float Akx = sel3(v0[0], v0[1], v0[2], s.kx) - okx, Aky = sel3(v0[0], v0[1], v0[2], s.ky) - oky,
                Akz = sel3(v0[0], v0[1], v0[2], s.kz) - okz;
    const float Bkx = sel3(v1[0], v1[1], v1[2], s.kx) - okx, Bky = sel3(v1[0], v1[1], v1[2], s.ky) - oky,
                Bkz = sel3(v1[0], v1[1], v1[2], s.kz) - okz;
    const float Ckx = sel3(v2[0], v2[1], v2[2], s.kx) - okx, Cky = sel3(v2[0], v2[1], v2[2], s.ky) - oky,
                Ckz = sel3(v2[0], v2[1], v2[2], s.kz) - okz;
    const float Ax = Akx - s.Sx * Akz, Ay = Aky - s.Sy * Akz;
    const float Bx = Bkx - s.Sx * Bkz, By = Bky - s.Sy * Bkz;
    const float Cx = Ckx - s.Sx * Ckz, Cy = Cky - s.Sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        U = rc_edge_double(Cx, By, Cy, Bx);
        V = rc_edge_double(Ax, Cy, Ay, Cx);
        W = rc_edge_double(Bx, Ay, By, Ax);
    }
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = (U + V) + W;
    if (det == 0.0f) return false;
    const float Az = s.Sz * Akz, Bz = s.Sz * Bkz, Cz = s.Sz * Ckz;
    float t = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t >= 0.0f) || !cell_finite(t)) return false;  // (a NaN fails t >= 0)
    if (t == 0.0f) t = 0.0f;                            // -0 -> +0: the key orders by the bits
    t_out = t;
    return true;
}
// the whole function as the header states it
__device__ __forceinline__ bool rc_intersect(const float (&o)[3], const float (&d)[3], const float *v0, const float *v1,
                                             const float *v2, float &t) {
    return rc_intersect_sheared(o, rc_shear(d[0], d[1], d[2]), v0, v1, v2, t);
}

struct RcMesh {
    const float *__restrict__ vertices;
    const int32_t *__restrict__ triangles;
    uint32_t V, T;
};
// one triangle against the ray, folded into the key.  Indices were checked by the build; they are clamped all the same so
// that a scene that skipped the check cannot read outside the vertex array.
__device__ __forceinline__ void rc_test(const RcMesh &m, uint32_t tri, const float (&o)[3], const RcShear &s,
                                        unsigned long long &best) {
    const int32_t *ix = m.triangles + (size_t)tri * 3;
    const uint32_t i0 = min((uint32_t)ix[0], m.V - 1), i1 = min((uint32_t)ix[1], m.V - 1), i2 = min((uint32_t)ix[2], m.V - 1);
    float t;
    if (rc_intersect_sheared(o, s, m.vertices + (size_t)i0 * 3, m.vertices + (size_t)i1 * 3, m.vertices + (size_t)i2 * 3, t)) {
        const unsigned long long key = (unsigned long long)__float_as_uint(t) << 32 | tri;
        best = key < best ? key : best;
    }
}

// --------------------------------------------------------------------------------------------------------------- bounds
__global__ void __launch_bounds__(kRcThreads)
k_rc_bounds(RcMesh m, uint32_t *__restrict__ partials) {
    const float inf = __uint_as_float(0x7f800000u);
    float f[9] = {inf, inf, inf, -inf, -inf, -inf, 0.0f, 0.0f, 0.0f};  // lo, hi, largest triangle extent
    uint32_t bad[2] = {0, 0};                                           // coordinates, indices
    cell_bounds_accumulate(m.vertices, m.V, f, f + 3, bad[0]);
    const uint32_t stride = gridDim.x * kRcThreads;
    for (uint32_t t = blockIdx.x * kRcThreads + threadIdx.x; t < m.T; t += stride) {  // (t + stride < 2^32: T < 2^31, stride <= 2^18)
        const int32_t *ix = m.triangles + (size_t)t * 3;
        const uint32_t i0 = (uint32_t)ix[0], i1 = (uint32_t)ix[1], i2 = (uint32_t)ix[2];
        const uint32_t out = (i0 >= m.V) + (i1 >= m.V) + (i2 >= m.V);  // (a negative index is a large unsigned one)
        bad[1] += out;
        if (out == 0) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float x0 = m.vertices[(size_t)i0 * 3 + a], x1 = m.vertices[(size_t)i1 * 3 + a],
                            x2 = m.vertices[(size_t)i2 * 3 + a];
                f[6 + a] = fmaxf(f[6 + a], fmaxf(fmaxf(x0, x1), x2) - fminf(fminf(x0, x1), x2));  // (fmaxf drops a NaN)
            }
        }
    }
    cell_block_reduce(f, bad, partials + (size_t)blockIdx.x * kRcBoundsWords);
}

__global__ void __launch_bounds__(kRcThreads)
k_rc_bounds_finish(const uint32_t *__restrict__ partials, uint32_t G, float *__restrict__ box, uint32_t *__restrict__ counts) {
    const float inf = __uint_as_float(0x7f800000u);
    float f[9] = {inf, inf, inf, -inf, -inf, -inf, 0.0f, 0.0f, 0.0f};
    uint32_t bad[2] = {0, 0};
    cell_merge_partials(partials, G, f, bad);
    __shared__ uint32_t s_out[kRcBoundsWords];
    cell_block_reduce(f, bad, s_out);
    __syncthreads();
    if (threadIdx.x < 9) box[threadIdx.x] = __uint_as_float(s_out[threadIdx.x]);
    if (threadIdx.x == 0) counts[0] = s_out[9], counts[1] = s_out[10], counts[2] = 0u, counts[3] = 0u;
}

// ------------------------------------------------------------------------------------------------------------ the lists
struct RcRange {
    uint32_t c0[3], c1[3];
};
__device__ __forceinline__ RcRange rc_triangle_cells(const RcMesh &m, const RcGrid &g, uint32_t tri) {
    const int32_t *ix = m.triangles + (size_t)tri * 3;
    const uint32_t i0 = min((uint32_t)ix[0], m.V - 1), i1 = min((uint32_t)ix[1], m.V - 1), i2 = min((uint32_t)ix[2], m.V - 1);
    RcRange r;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float x0 = m.vertices[(size_t)i0 * 3 + a], x1 = m.vertices[(size_t)i1 * 3 + a], x2 = m.vertices[(size_t)i2 * 3 + a];
        r.c0[a] = cell_of(fminf(fminf(x0, x1), x2) - g.delta[a], g.lo[a], g.inv[a], g.n[a]);
        r.c1[a] = cell_of(fmaxf(fmaxf(x0, x1), x2) + g.delta[a], g.lo[a], g.inv[a], g.n[a]);
        if (r.c1[a] < r.c0[a]) r.c1[a] = r.c0[a];  // (cannot happen for finite vertices: cell_of is monotone)
    }
    return r;
}

__global__ void __launch_bounds__(kRcThreads)
k_rc_count(RcMesh m, const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t *__restrict__ cell_count) {
    const uint32_t tri = blockIdx.x * kRcThreads + threadIdx.x;
    if (tri >= m.T) return;
    const RcGrid g = rc_grid(box, nx, ny, nz);
    const RcRange r = rc_triangle_cells(m, g, tri);
    for (uint32_t x = r.c0[0]; x <= r.c1[0]; x++)
        for (uint32_t y = r.c0[1]; y <= r.c1[1]; y++)
            for (uint32_t z = r.c0[2]; z <= r.c1[2]; z++) atomicAdd(&cell_count[(x * ny + y) * nz + z], 1u);  // < cells
}

// exclusive scan of cell_count[cells] -> cell_start[cells + 1] (32 bits, wrapping), the 64-bit total -> counts[2], counts[3]
__global__ void __launch_bounds__(kScanThreads)
k_rc_scan(const uint32_t *__restrict__ cell_count, uint32_t cells, uint32_t *__restrict__ cell_start, uint32_t *__restrict__ counts) {
    // 64 bits from the sum of a thread's cells to the total: a single tile of cells can list more than 2^32 entries
    const unsigned long long total = workgroup_scan<unsigned long long>(
        cells, 0ull, [&](uint32_t c, bool) { return cell_count[c]; },
        [&](uint32_t c, unsigned long long at) { cell_start[c] = (uint32_t)at; });
    if (threadIdx.x == 0) {
        cell_start[cells] = (uint32_t)total;
        counts[2] = (uint32_t)total, counts[3] = (uint32_t)(total >> 32);
    }
}

__global__ void __launch_bounds__(kRcThreads)
k_rc_fill(RcMesh m, const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *__restrict__ cell_start,
          uint32_t *__restrict__ cursor, uint32_t *__restrict__ cell_tris, uint32_t entries) {
    const uint32_t tri = blockIdx.x * kRcThreads + threadIdx.x;
    if (tri >= m.T) return;
    const RcGrid g = rc_grid(box, nx, ny, nz);
    const RcRange r = rc_triangle_cells(m, g, tri);
    for (uint32_t x = r.c0[0]; x <= r.c1[0]; x++)
        for (uint32_t y = r.c0[1]; y <= r.c1[1]; y++)
            for (uint32_t z = r.c0[2]; z <= r.c1[2]; z++) {
                const uint32_t c = (x * ny + y) * nz + z;
                const uint32_t slot = cell_start[c] + atomicAdd(&cursor[c], 1u);
                if (slot < cell_start[c + 1] && slot < entries) cell_tris[slot] = tri;  // (never outside the buffer)
            }
}

// ------------------------------------------------------------------------------------------------------------- the cast
__global__ void __launch_bounds__(kRcCastThreads)
k_rc_cast(RcMesh m, const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *__restrict__ cell_start,
          const uint32_t *__restrict__ cell_tris, uint32_t entries, const float *__restrict__ rays_o,
          const float *__restrict__ rays_d, uint32_t N, float *__restrict__ t_hit, int32_t *__restrict__ prim_ids,
          float *__restrict__ prim_normals, float *__restrict__ incidences) {
    const uint32_t ray = blockIdx.x * kRcCastThreads + threadIdx.x;
    if (ray >= N) return;
    const float inf = __uint_as_float(0x7f800000u);
    const float o[3] = {rays_o[(size_t)ray * 3], rays_o[(size_t)ray * 3 + 1], rays_o[(size_t)ray * 3 + 2]};
    const float d[3] = {rays_d[(size_t)ray * 3], rays_d[(size_t)ray * 3 + 1], rays_d[(size_t)ray * 3 + 2]};
    unsigned long long best = ~0ull;
    const bool valid = cell_finite(o[0]) && cell_finite(o[1]) && cell_finite(o[2]) && cell_finite(d[0]) && cell_finite(d[1]) &&
                       cell_finite(d[2]) && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
    if (valid) {
        const RcShear s = rc_shear(d[0], d[1], d[2]);
        const RcGrid g = rc_grid(box, nx, ny, nz);
        // is the walk's arithmetic good to delta / 4 for this ray?
        float mag = 0.0f, dmax = 0.0f, dmin = inf, delta_min = inf;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            mag = fmaxf(mag, fmaxf(fmaxf(fabsf(g.lo[a]), fabsf(g.hi[a])), fabsf(o[a])));
            dmax = fmaxf(dmax, fabsf(d[a]));
            if (d[a] != 0.0f) dmin = fminf(dmin, fabsf(d[a]));
            delta_min = fminf(delta_min, g.delta[a]);
        }
        const float E = mag * kRcErrScale;
        const bool tame = (nx | ny | nz) > 1 && 4.0f * E <= delta_min && mag >= kRcSmall && mag <= kRcBig && dmax >= kRcSmall &&
                          dmax <= kRcBig && dmin >= 7.8886090522101181e-31f;  // 2^-100
        if (!tame) {
            for (uint32_t tri = 0; tri < m.T; tri++) rc_test(m, tri, o, s, best);
        } else {
            float invd[3], t0 = -inf, t1 = inf;
            bool miss = false;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float blo = g.lo[a] - g.delta[a], bhi = g.hi[a] + g.delta[a];
                invd[a] = d[a] != 0.0f ? 1.0f / d[a] : 0.0f;
                if (d[a] != 0.0f) {
                    const float ta = (blo - o[a]) * invd[a], tb = (bhi - o[a]) * invd[a];
                    t0 = fmaxf(t0, fminf(ta, tb));
                    t1 = fminf(t1, fmaxf(ta, tb));
                } else if (o[a] < blo || o[a] > bhi) {
                    miss = true;
                }
            }
            const float dz_abs = fabsf(sel3(d[0], d[1], d[2], s.kz));
            const float ext_kz = sel3(g.maxext[0], g.maxext[1], g.maxext[2], s.kz), delta_kz = sel3(g.delta[0], g.delta[1], g.delta[2], s.kz);
            const float tau = (ext_kz * 1.001f + delta_kz) / dz_abs;
            const float ts = fmaxf(t0, -tau);
            if (!miss && ts <= t1) {
                uint32_t ic[3];
                float tn[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const float p = d[a] != 0.0f ? o[a] + ts * d[a] : o[a];
                    ic[a] = cell_of(p, g.lo[a], g.inv[a], g.n[a]);
                }
                // parameter at which the ray crosses the far plane of cell k along axis a; the outermost planes are the
                // dilated box's, so the boundary cells own the shell around the box
                auto t_next = [&](int a, uint32_t k) -> float {
                    if (d[a] == 0.0f) return inf;
                    const uint32_t plane = d[a] > 0.0f ? k + 1 : k;
                    const float x = plane == 0 ? g.lo[a] - g.delta[a]
                                               : (plane == g.n[a] ? g.hi[a] + g.delta[a] : g.lo[a] + (float)plane * g.w[a]);
                    return (x - o[a]) * invd[a];
                };
#pragma unroll
                for (int a = 0; a < 3; a++) tn[a] = t_next(a, ic[a]);
                const uint32_t max_steps = nx + ny + nz + 3;
                for (uint32_t step = 0; step < max_steps; step++) {
                    const uint32_t c = (ic[0] * ny + ic[1]) * nz + ic[2];
                    const uint32_t e0 = min(cell_start[c], entries), e1 = min(cell_start[c + 1], entries);
                    for (uint32_t e = e0; e < e1; e++) rc_test(m, min(cell_tris[e], m.T - 1), o, s, best);
                    const uint32_t axis = (tn[0] <= tn[1] && tn[0] <= tn[2]) ? 0u : (tn[1] <= tn[2] ? 1u : 2u);
                    const float t_exit = sel3(tn[0], tn[1], tn[2], axis);
                    if (best != ~0ull && __uint_as_float((uint32_t)(best >> 32)) + tau <= t_exit) break;
                    if (!(t_exit < inf)) break;
                    // one step along `axis`, with selects: no runtime-indexed registers
                    const bool up = sel3(d[0], d[1], d[2], axis) > 0.0f;
                    const uint32_t cur = axis == 0 ? ic[0] : (axis == 1 ? ic[1] : ic[2]);
                    const uint32_t lim = axis == 0 ? nx : (axis == 1 ? ny : nz);
                    if (up ? cur + 1 >= lim : cur == 0) break;
                    const uint32_t nxt = up ? cur + 1 : cur - 1;
                    if (axis == 0) ic[0] = nxt, tn[0] = t_next(0, nxt);
                    else if (axis == 1) ic[1] = nxt, tn[1] = t_next(1, nxt);
                    else ic[2] = nxt, tn[2] = t_next(2, nxt);
                }
            }
        }
    }
    float t = inf, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f, inc = 0.0f;
    int32_t id = -1;
    if (best != ~0ull) {
        t = __uint_as_float((uint32_t)(best >> 32));
        id = (int32_t)(uint32_t)best;
        const int32_t *ix = m.triangles + (size_t)id * 3;
        const uint32_t i0 = min((uint32_t)ix[0], m.V - 1), i1 = min((uint32_t)ix[1], m.V - 1), i2 = min((uint32_t)ix[2], m.V - 1);
        const float *a = m.vertices + (size_t)i0 * 3, *b = m.vertices + (size_t)i1 * 3, *c = m.vertices + (size_t)i2 * 3;
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
        const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
        const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
        const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
        if (len > 0.0f && cell_finite(len)) {
            n0 = cx / len, n1 = cy / len, n2 = cz / len;
            inc = fabsf((d[0] * n0 + d[1] * n1) + d[2] * n2);
        }
    }
    t_hit[ray] = t;
    prim_ids[ray] = id;
    prim_normals[(size_t)ray * 3] = n0, prim_normals[(size_t)ray * 3 + 1] = n1, prim_normals[(size_t)ray * 3 + 2] = n2;
    if (incidences) incidences[ray] = inc;
}

// ------------------------------------------------------------------------------------------------------------ host side
uint32_t rc_bounds_groups(uint32_t V, uint32_t T) { return cell_bounds_groups(V > T ? V : T); }
uint64_t rc_ws_bytes(uint32_t V, uint32_t T, uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint64_t bounds = 4ull * kRcBoundsWords * rc_bounds_groups(V, T), cells = 4ull * nx * ny * nz;
    return ((bounds > cells ? bounds : cells) + 15) & ~15ull;
}
int rc_check_mesh(const char *who, const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T) {
    LNH_REQUIRE(vertices && triangles, LNH_ERR_INVALID_ARG, "%s: null pointer (vertices / triangles)", who);
    LNH_REQUIRE(V >= 1 && T >= 1, LNH_ERR_INVALID_ARG, "%s: empty mesh (%u vertices, %u triangles)", who, V, T);
    LNH_REQUIRE(V < (1u << 31) && T < (1u << 31), LNH_ERR_UNSUPPORTED, "%s: %u vertices / %u triangles, indices are int32 (< 2^31)",
                who, V, T);
    return LNH_OK;
}
int rc_check_ws(const char *who, uint32_t V, uint32_t T, uint32_t nx, uint32_t ny, uint32_t nz, const void *ws, uint64_t ws_bytes) {
    return cell_check_ws(who, rc_ws_bytes(V, T, nx, ny, nz), ws, ws_bytes);
}

}  // namespace

extern "C" {

uint64_t lnh_raycast_workspace_size(uint32_t V, uint32_t T, uint32_t nx, uint32_t ny, uint32_t nz, uint64_t entries) {
    if (V < 1 || T < 1 || V >= (1u << 31) || T >= (1u << 31) || !cell_grid_ok(nx, ny, nz) || entries > 0x7fffffffull) return 0;
    return rc_ws_bytes(V, T, nx, ny, nz);
}

int lnh_raycast_bounds(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, void *ws, uint64_t ws_bytes,
                       float *box, uint32_t *counts, lnh_stream_t stream) {
    int rc = rc_check_mesh("raycast_bounds", vertices, V, triangles, T);
    if (rc) return rc;
    LNH_REQUIRE(box && counts && ((uintptr_t)box & 3) == 0 && ((uintptr_t)counts & 3) == 0, LNH_ERR_INVALID_ARG,
                "raycast_bounds: null pointer (box / counts)");
    if ((rc = rc_check_ws("raycast_bounds", V, T, 1, 1, 1, ws, ws_bytes))) return rc;
    const RcMesh m = {vertices, triangles, V, T};
    const uint32_t G = rc_bounds_groups(V, T);
    hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_rc_bounds, dim3(G), dim3(kRcThreads), 0, s, m, (uint32_t *)ws);
    if ((rc = lnh_check_launch("lnh_raycast_bounds(partials)"))) return rc;
    LNH_LAUNCH(k_rc_bounds_finish, dim3(1), dim3(kRcThreads), 0, s, (const uint32_t *)ws, G, box, counts);
    return lnh_check_launch("lnh_raycast_bounds(finish)");
}

int lnh_raycast_build_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *box,
                            uint32_t nx, uint32_t ny, uint32_t nz, void *ws, uint64_t ws_bytes, uint32_t *cell_start,
                            uint32_t *counts, lnh_stream_t stream) {
    int rc = rc_check_mesh("raycast_build_count", vertices, V, triangles, T);
    if (rc) return rc;
    if ((rc = cell_check_grid("raycast_build_count", box, nx, ny, nz))) return rc;
    LNH_REQUIRE(cell_start && counts && ((uintptr_t)cell_start & 3) == 0 && ((uintptr_t)counts & 3) == 0, LNH_ERR_INVALID_ARG,
                "raycast_build_count: null pointer (cell_start / counts)");
    if ((rc = rc_check_ws("raycast_build_count", V, T, nx, ny, nz, ws, ws_bytes))) return rc;
    const RcMesh m = {vertices, triangles, V, T};
    const uint32_t cells = nx * ny * nz;  // <= 2^30
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lnh_zero_async(ws, 4ull * cells, s, "lnh_raycast_build_count(clear)"))) return rc;
    LNH_LAUNCH(k_rc_count, dim3(div_up(T, kRcThreads)), dim3(kRcThreads), 0, s, m, box, nx, ny, nz, (uint32_t *)ws);
    if ((rc = lnh_check_launch("lnh_raycast_build_count(count)"))) return rc;
    LNH_LAUNCH(k_rc_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)ws, cells, cell_start, counts);
    return lnh_check_launch("lnh_raycast_build_count(scan)");
}

int lnh_raycast_build_fill(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *box,
                           uint32_t nx, uint32_t ny, uint32_t nz, void *ws, uint64_t ws_bytes, const uint32_t *cell_start,
                           uint32_t *cell_tris, uint64_t entries, lnh_stream_t stream) {
    int rc = rc_check_mesh("raycast_build_fill", vertices, V, triangles, T);
    if (rc) return rc;
    if ((rc = cell_check_grid("raycast_build_fill", box, nx, ny, nz))) return rc;
    LNH_REQUIRE(cell_start && cell_tris && ((uintptr_t)cell_start & 3) == 0 && ((uintptr_t)cell_tris & 3) == 0, LNH_ERR_INVALID_ARG,
                "raycast_build_fill: null pointer (cell_start / cell_tris)");
    LNH_REQUIRE(entries >= 1, LNH_ERR_INVALID_ARG, "raycast_build_fill: %llu entries: every triangle is listed at least once",
                (unsigned long long)entries);
    LNH_REQUIRE(entries <= 0x7fffffffull, LNH_ERR_UNSUPPORTED,
                "raycast_build_fill: %llu entries, the lists hold at most 2^31 - 1 (use a coarser grid)", (unsigned long long)entries);
    if ((rc = rc_check_ws("raycast_build_fill", V, T, nx, ny, nz, ws, ws_bytes))) return rc;
    const RcMesh m = {vertices, triangles, V, T};
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lnh_zero_async(ws, 4ull * nx * ny * nz, s, "lnh_raycast_build_fill(clear)"))) return rc;
    LNH_LAUNCH(k_rc_fill, dim3(div_up(T, kRcThreads)), dim3(kRcThreads), 0, s, m, box, nx, ny, nz, cell_start, (uint32_t *)ws, cell_tris,
               (uint32_t)entries);
    return lnh_check_launch("lnh_raycast_build_fill");
}

int lnh_raycast_cast(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *box, uint32_t nx,
                     uint32_t ny, uint32_t nz, const uint32_t *cell_start, const uint32_t *cell_tris, uint64_t entries,
                     const float *rays_o, const float *rays_d, uint32_t N, float *t_hit, int32_t *primitive_ids,
                     float *primitive_normals, float *incidences, lnh_stream_t stream) {
    int rc = rc_check_mesh("raycast_cast", vertices, V, triangles, T);
    if (rc) return rc;
    if ((rc = cell_check_grid("raycast_cast", box, nx, ny, nz))) return rc;
    LNH_REQUIRE(cell_start && cell_tris && ((uintptr_t)cell_start & 3) == 0 && ((uintptr_t)cell_tris & 3) == 0, LNH_ERR_INVALID_ARG,
                "raycast_cast: null pointer (cell_start / cell_tris)");
    LNH_REQUIRE(entries >= 1, LNH_ERR_INVALID_ARG, "raycast_cast: %llu entries: the scene was not built",
                (unsigned long long)entries);
    LNH_REQUIRE(entries <= 0x7fffffffull, LNH_ERR_UNSUPPORTED, "raycast_cast: %llu entries, the lists hold at most 2^31 - 1",
                (unsigned long long)entries);
    if (N == 0) return LNH_OK;
    LNH_REQUIRE(N < (1u << 31), LNH_ERR_UNSUPPORTED, "raycast_cast: %u rays, at most 2^31 - 1 per call", N);
    LNH_REQUIRE(rays_o && rays_d && t_hit && primitive_ids && primitive_normals, LNH_ERR_INVALID_ARG,
                "raycast_cast: null pointer (rays_o / rays_d / t_hit / primitive_ids / primitive_normals)");
    const RcMesh m = {vertices, triangles, V, T};
    LNH_LAUNCH(k_rc_cast, dim3(div_up(N, kRcCastThreads)), dim3(kRcCastThreads), 0, (hipStream_t)stream, m, box, nx, ny, nz, cell_start,
               cell_tris, (uint32_t)entries, rays_o, rays_d, N, t_hit, primitive_ids, primitive_normals, incidences);
    return lnh_check_launch("lnh_raycast_cast");
}

}  // extern "C"
