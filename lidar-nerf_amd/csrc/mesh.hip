// mesh.hip — marching cubes over a density volume on the GPU: the second half of Trainer.save_mesh.
// Replaces extract_geometry / mcubes.marching_cubes, nerf/utils.py:169-184 (PyMCubes on the host over a NumPy volume).
//
// volume: fp32 [nx, ny, nz], z fastest (the reference's u[x, y, z]).  A corner is BELOW iff v < iso (a NaN is not below);
// an edge crosses iff exactly one end is below.  The 256 cases come from mc_tables.h (gen_mc_tables.py: numbering of
// corners and edges, the face rule, the winding).
//
// Output contract (the order is fixed; tests compare bit for bit):
//   vertex   owned by the lattice point at the lower end of its edge; every point owns its +x, +y, +z edges.  Vertices are in
//            lattice-point order (flattened [x, y, z]), within a point x, then y, then z edge; a vertex shared by up to four
//            cells appears once.  Position in index units: t = (iso - va) / (vb - va), moving coordinate float(i) + t (fp32,
//            the library is built with -ffp-contract=off).
//   triangle in cell order (flattened [x, y, z] over (nx-1)(ny-1)(nz-1) cells), within a cell the table's order.
//
// Passes, one thread per lattice point, 256 points per workgroup, no atomics of any kind:
//   k_mc_count      case of the point's cell, its triangle count, its 0-3 owned crossing edges, non-finite sample -> ONE packed
//                   word of totals per workgroup
//   k_mc_scan       ONE workgroup: exclusive scans of the workgroup totals (vertices, triangles) side by side with scan.h's
//                   workgroup_scan; writes counts[4]
//   k_mc_vertices   case again, scan inside the workgroup -> every point's global vertex offset (workspace) and the vertices
//   k_mc_triangles  case again, scan inside the workgroup -> the triangles; a corner is the owner's vertex offset + the rank
//                   of the edge among that owner's crossing edges.  Owners live in other workgroups, hence the launch boundary
//                   between the last two passes; no workgroup ever waits for another.
// Workspace: totals u32[G] | vertex offset of the workgroup u32[G] | triangle offset u32[G] | vertex offset of the point u32[N],
// G = ceil(N / 256).
#include "common.h"
#include "mc_tables.h"
#include "scan.h"

namespace {

constexpr uint32_t kMcThreads = 256;
// packed per-workgroup totals: vertices (<= 3 * 256) in bits 0-9, triangles (<= kMcMaxTriangles * 256) in bits 10-20,
// non-finite samples (<= 256) in bits 21-29
constexpr uint32_t kMcTriShift = 10, kMcBadShift = 21;
static_assert(3 * kMcThreads < (1u << kMcTriShift), "vertex total of a workgroup must fit its field");
static_assert(kMcMaxTriangles * kMcThreads < (1u << (kMcBadShift - kMcTriShift)), "per-cell bound against the table's maximum");
static_assert(kMcMaxTriangles <= 5, "k_mc_triangles writes at most 5 triangles per cell");

struct McDims {
    uint32_t nx, ny, nz, n;  // n = nx * ny * nz < 2^31
};

// What a lattice point knows: its cell's case (valid iff `cell`), the values at the 8 corners (a corner beyond the volume
// repeats the nearer one, so an edge that does not exist never crosses) and the crossing flags of its three owned edges.
struct McPoint {
    uint32_t x, y, z, kase;
    bool cell, cx, cy, cz;
    float v0, vx, vy, vz;
};
__device__ __forceinline__ McPoint mc_point(const float *__restrict__ vol, const McDims &d, uint32_t p, float iso) {
    McPoint q;
    q.z = p % d.nz;
    const uint32_t xy = p / d.nz;
    q.y = xy % d.ny;
    q.x = xy / d.ny;
    const uint32_t sx = q.x + 1 < d.nx ? d.ny * d.nz : 0u, sy = q.y + 1 < d.ny ? d.nz : 0u, sz = q.z + 1 < d.nz ? 1u : 0u;
    q.cell = sx && sy && sz;
    float v[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) v[i] = vol[p + (i & 1) * sx + ((i >> 1) & 1) * sy + (i >> 2) * sz];  // every index < n
    q.kase = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) q.kase |= (v[i] < iso ? 1u : 0u) << i;
    const uint32_t b0 = q.kase & 1;
    q.cx = ((q.kase >> 1) & 1) != b0;
    q.cy = ((q.kase >> 2) & 1) != b0;
    q.cz = ((q.kase >> 4) & 1) != b0;
    q.v0 = v[0], q.vx = v[1], q.vy = v[2], q.vz = v[4];
    return q;
}

__global__ void __launch_bounds__(kMcThreads)
k_mc_count(const float *__restrict__ vol, McDims d, float iso, uint32_t *__restrict__ wg_totals) {
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * kMcThreads + threadIdx.x;
    uint32_t packed = 0;
    if (p < d.n) {
        const McPoint q = mc_point(vol, d, p, iso);
        const uint32_t nv = (uint32_t)q.cx + q.cy + q.cz, nt = q.cell ? kMcTriCount[q.kase] : 0u;
        const uint32_t bad = (__float_as_uint(q.v0) & 0x7f800000u) == 0x7f800000u;  // inf or NaN
        packed = nv | nt << kMcTriShift | bad << kMcBadShift;
    }
    uint32_t total;
    (void)block_scan_256(packed, s_wave, total);  // (the fields cannot carry into each other: static_asserts above)
    if (threadIdx.x == 0) wg_totals[blockIdx.x] = total;
}

// the two sums k_mc_scan forms side by side (vertices, triangles): 32 bits inside a tile of 4096 workgroups of 256 points,
// 64 bits over the tiles
struct McSums {
    uint32_t v, t;
    __device__ __forceinline__ McSums &operator+=(const McSums &o) { return v += o.v, t += o.t, *this; }
};
__device__ __forceinline__ McSums operator+(McSums a, const McSums &b) { return a += b; }
__device__ __forceinline__ McSums operator-(const McSums &a, const McSums &b) { return {a.v - b.v, a.t - b.t}; }
__device__ __forceinline__ McSums scan_wave(const McSums &s) { return {::scan_wave(s.v), ::scan_wave(s.t)}; }
__device__ __forceinline__ McSums scan_lane(const McSums &s, uint32_t lane) { return {::scan_lane(s.v, lane), ::scan_lane(s.t, lane)}; }
struct McTotals {
    unsigned long long v, t;
    __device__ __forceinline__ McTotals &operator+=(const McSums &o) { return v += o.v, t += o.t, *this; }
};
__device__ __forceinline__ McTotals operator+(McTotals a, const McSums &b) { return a += b; }

__global__ void __launch_bounds__(kScanThreads)
k_mc_scan(const uint32_t *__restrict__ wg_totals, uint32_t G, uint32_t *__restrict__ wg_voff, uint32_t *__restrict__ wg_toff,
          uint32_t *__restrict__ counts) {
    constexpr uint32_t kWaves = kScanThreads / 64;
    __shared__ uint32_t s_b[kWaves];
    uint32_t my_bad = 0;  // non-finite samples of the workgroups this thread loads: summed once, behind the scan
    const McTotals end = workgroup_scan<McTotals, McSums>(
        G, McTotals{0, 0},
        [&](uint32_t g, bool live) {
            const uint32_t w = wg_totals[g];
            my_bad += live ? w >> kMcBadShift : 0u;
            return McSums{w & ((1u << kMcTriShift) - 1), (w >> kMcTriShift) & ((1u << (kMcBadShift - kMcTriShift)) - 1)};
        },
        [&](uint32_t g, const McTotals &off) { wg_voff[g] = (uint32_t)off.v, wg_toff[g] = (uint32_t)off.t; });
    const uint32_t ib = wave_scan_add_u32(my_bad);
    if ((threadIdx.x & 63) == 63) s_b[threadIdx.x >> 6] = ib;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t bad = 0;
        for (uint32_t w = 0; w < kWaves; w++) bad += s_b[w];
        // a count that does not fit 32 bits saturates: the caller refuses it (the offsets above have wrapped)
        counts[0] = end.v > 0xffffffffull ? 0xffffffffu : (uint32_t)end.v;
        counts[1] = end.t > 0xffffffffull ? 0xffffffffu : (uint32_t)end.t;
        counts[2] = bad;
        counts[3] = 0u;
    }
}

__global__ void __launch_bounds__(kMcThreads)
k_mc_vertices(const float *__restrict__ vol, McDims d, float iso, const uint32_t *__restrict__ wg_voff,
              uint32_t *__restrict__ point_voff, float *__restrict__ vertices, uint32_t max_vertices) {
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * kMcThreads + threadIdx.x;
    McPoint q;
    uint32_t nv = 0;
    if (p < d.n) {
        q = mc_point(vol, d, p, iso);
        nv = (uint32_t)q.cx + q.cy + q.cz;
    }
    uint32_t total;
    uint32_t k = wg_voff[blockIdx.x] + block_scan_256(nv, s_wave, total);
    if (p >= d.n) return;
    point_voff[p] = k;
    if (nv == 0) return;
    const float fx = (float)q.x, fy = (float)q.y, fz = (float)q.z;
    if (q.cx) {
        if (k < max_vertices) {
            float *o = vertices + (size_t)k * 3;
            o[0] = fx + (iso - q.v0) / (q.vx - q.v0), o[1] = fy, o[2] = fz;
        }
        k++;
    }
    if (q.cy) {
        if (k < max_vertices) {
            float *o = vertices + (size_t)k * 3;
            o[0] = fx, o[1] = fy + (iso - q.v0) / (q.vy - q.v0), o[2] = fz;
        }
        k++;
    }
    if (q.cz && k < max_vertices) {
        float *o = vertices + (size_t)k * 3;
        o[0] = fx, o[1] = fy, o[2] = fz + (iso - q.v0) / (q.vz - q.v0);
    }
}

__global__ void __launch_bounds__(kMcThreads)
k_mc_triangles(const float *__restrict__ vol, McDims d, float iso, const uint32_t *__restrict__ wg_toff,
               const uint32_t *__restrict__ point_voff, int32_t *__restrict__ triangles, uint32_t max_triangles) {
    __shared__ uint32_t s_wave[4];
    const uint32_t p = blockIdx.x * kMcThreads + threadIdx.x;
    McPoint q;
    uint32_t nt = 0;
    if (p < d.n) {
        q = mc_point(vol, d, p, iso);
        nt = q.cell ? kMcTriCount[q.kase] : 0u;
    }
    uint32_t total;
    const uint32_t first = wg_toff[blockIdx.x] + block_scan_256(nt, s_wave, total);
    if (nt == 0) return;  // (nt > 0: the point has a cell, so all 8 corners are distinct lattice points)
    const uint32_t sx = d.ny * d.nz, sy = d.nz;
    for (uint32_t j = 0; j < nt; j++) {
        if (first + j >= max_triangles) return;
        int32_t *o = triangles + (size_t)(first + j) * 3;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            const uint32_t e = (uint32_t)kMcTriEdges[q.kase][3 * j + c], axis = e >> 2, k = e & 3;
            // lower corner of the edge = the owner: offsets of the two other axes, in increasing axis order
            const uint32_t ox = axis == 0 ? 0u : (k & 1), oy = axis == 0 ? (k & 1) : (axis == 1 ? 0u : (k >> 1)),
                           oz = axis == 2 ? 0u : (k >> 1);
            const uint32_t owner = p + ox * sx + oy * sy + oz;  // a corner of this cell: < n
            const bool below = (q.kase >> (ox | oy << 1 | oz << 2)) & 1;
            // rank of the edge among the owner's crossing edges: its x edge (axis >= 1) and y edge (axis == 2) come first;
            // their far ends may lie outside this cell, but inside the volume when the edge exists
            uint32_t rank = 0;
            if (axis >= 1 && q.x + ox + 1 < d.nx) rank += ((vol[owner + sx] < iso) != below) ? 1u : 0u;
            if (axis == 2 && q.y + oy + 1 < d.ny) rank += ((vol[owner + sy] < iso) != below) ? 1u : 0u;
            o[c] = (int32_t)(point_voff[owner] + rank);
        }
    }
}

struct McLayout {
    uint64_t totals, voff, toff, point_voff, bytes;
    uint32_t groups;
};
bool mc_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const uint64_t xy = (uint64_t)nx * ny;  // < 2^64
    return xy < (1ull << 31) && xy * nz < (1ull << 31);
}
McLayout mc_layout(uint64_t n) {
    McLayout l;
    l.groups = div_up(n, kMcThreads);
    l.totals = 0;
    l.voff = l.totals + 4ull * l.groups;
    l.toff = l.voff + 4ull * l.groups;
    l.point_voff = l.toff + 4ull * l.groups;
    l.bytes = (l.point_voff + 4ull * n + 15) & ~15ull;
    return l;
}

int mc_check(const char *who, const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, const void *ws,
             uint64_t ws_bytes) {
    LNH_REQUIRE(volume && ws, LNH_ERR_INVALID_ARG, "%s: null pointer", who);
    LNH_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, LNH_ERR_INVALID_ARG, "%s: volume of %u x %u x %u samples, every dimension must be >= 2",
                who, nx, ny, nz);
    LNH_REQUIRE(mc_dims_ok(nx, ny, nz), LNH_ERR_UNSUPPORTED, "%s: %u x %u x %u samples, point indices are 31 bits wide (nx*ny*nz < 2^31)",
                who, nx, ny, nz);
    LNH_REQUIRE(iso == iso, LNH_ERR_INVALID_ARG, "%s: iso is NaN", who);
    const McLayout l = mc_layout((uint64_t)nx * ny * nz);
    LNH_REQUIRE(((uintptr_t)ws & 3) == 0 && ws_bytes >= l.bytes, LNH_ERR_INVALID_ARG,
                "%s: workspace of %llu bytes (4-byte aligned) needed, got %llu", who, (unsigned long long)l.bytes,
                (unsigned long long)ws_bytes);
    return LNH_OK;
}

}  // namespace

extern "C" {

uint64_t lnh_marching_cubes_workspace_size(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (!mc_dims_ok(nx, ny, nz)) return 0;
    return mc_layout((uint64_t)nx * ny * nz).bytes;
}

int lnh_marching_cubes_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *ws, uint64_t ws_bytes,
                             uint32_t *counts, lnh_stream_t stream) {
    int rc = mc_check("marching_cubes_count", volume, nx, ny, nz, iso, ws, ws_bytes);
    if (rc) return rc;
    LNH_REQUIRE(counts && ((uintptr_t)counts & 3) == 0, LNH_ERR_INVALID_ARG, "marching_cubes_count: null pointer (counts)");
    const McDims d = {nx, ny, nz, nx * ny * nz};
    const McLayout l = mc_layout(d.n);
    char *w = (char *)ws;
    uint32_t *totals = (uint32_t *)(w + l.totals), *voff = (uint32_t *)(w + l.voff), *toff = (uint32_t *)(w + l.toff);
    hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_mc_count, dim3(l.groups), dim3(kMcThreads), 0, s, volume, d, iso, totals);
    if ((rc = lnh_check_launch("lnh_marching_cubes_count(count)"))) return rc;
    LNH_LAUNCH(k_mc_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)totals, l.groups, voff, toff, counts);
    return lnh_check_launch("lnh_marching_cubes_count(scan)");
}

int lnh_marching_cubes_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *ws, uint64_t ws_bytes,
                            float *vertices, uint32_t max_vertices, int32_t *triangles, uint32_t max_triangles,
                            lnh_stream_t stream) {
    int rc = mc_check("marching_cubes_emit", volume, nx, ny, nz, iso, ws, ws_bytes);
    if (rc) return rc;
    LNH_REQUIRE(vertices && triangles, LNH_ERR_INVALID_ARG, "marching_cubes_emit: null pointer (vertices / triangles)");
    LNH_REQUIRE(max_vertices >= 1 && max_triangles >= 1, LNH_ERR_INVALID_ARG,
                "marching_cubes_emit: capacity of %u vertices and %u triangles: an empty mesh needs no call", max_vertices,
                max_triangles);
    LNH_REQUIRE(max_vertices < (1u << 31), LNH_ERR_UNSUPPORTED,
                "marching_cubes_emit: max_vertices = %u, triangle indices are int32", max_vertices);
    const McDims d = {nx, ny, nz, nx * ny * nz};
    const McLayout l = mc_layout(d.n);
    char *w = (char *)ws;
    const uint32_t *voff = (const uint32_t *)(w + l.voff), *toff = (const uint32_t *)(w + l.toff);
    uint32_t *point_voff = (uint32_t *)(w + l.point_voff);
    hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_mc_vertices, dim3(l.groups), dim3(kMcThreads), 0, s, volume, d, iso, voff, point_voff, vertices, max_vertices);
    if ((rc = lnh_check_launch("lnh_marching_cubes_emit(vertices)"))) return rc;
    LNH_LAUNCH(k_mc_triangles, dim3(l.groups), dim3(kMcThreads), 0, s, volume, d, iso, toff, (const uint32_t *)point_voff,
               triangles, max_triangles);
    return lnh_check_launch("lnh_marching_cubes_emit(triangles)");
}

}  // extern "C"
