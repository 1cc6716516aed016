// tsdf.hip — projective TSDF fusion of range images into a lattice, and the mesh trim that follows marching cubes: the meshing
// function of the mesh baseline's fit (LidarNVSMeshing.fit of lidarnvs/lidarnvs_meshing.py takes a `meshing_func`; this is the
// one that suits a training sequence of range images with poses — DESIGN §20 says why it is not the reference's Poisson recipe).
//
// Lattice: point (ix, iy, iz) sits at lo + float(i) * step per axis; arrays are [nx, ny, nz], z fastest — the layout
// lnh_marching_cubes_* reads.  All arithmetic is fp32, one rounded operation per operator, nothing contracted
// (-ffp-contract=off); atan2 alone is taken in double and rounded (pano_geom.h).
//
// k_tsdf_integrate   one thread owns a lattice point and walks the frames 0 .. F-1 itself:
//     p  = lo + float(i) * step                                   (per axis)
//     q  = ((m0 * px + m1 * py) + m2 * pz) + m3                   (per row of the frame's 3 x 4 world -> lidar matrix)
//     r, pixel = pano_pixel_xyz<wrap>(q)                          (r = sqrt((qx qx + qy qy) + qz qz); skip unless 0 < r < max_depth,
//                                                                  skip outside the rows; column W is column 0)
//     d  = pano[f][pixel]; skip unless 0 < d < inf
//     s  = d - r; skip if s < -trunc
//     sum += min(s / trunc, 1); count += 1
//   No atomics, no thread reads another's result: (sum, count) after the call is a function of (sum, count) before it and the
//   inputs, and frames split over several calls give the bits of one call.  The matrices are indexed by the loop counter alone, so
//   they are scalar loads; the depth gather is the one irregular access, and a wave covers a 4 x 4 x 4 brick of lattice points
//   (a workgroup four of them stacked in z) so that its 64 pixels of a frame are neighbours.  (64 consecutive z per wave was
//   tried and measured 1 % slower; it is not kept.)
// k_tsdf_finalize    volume = count >= min_count ? -(sum / float(count)) : kTsdfFill.  Free space is negative, i.e. the BELOW side
//   of marching cubes at iso 0, so the mesh normals face the sensors.  kTsdfFill = +1, the value of a point every frame saw deep
//   behind a surface's band would have if it were counted: unobserved points are all equal, so a cell made only of them never crosses.
// k_mesh_vertex_observed   keep[v] = every lattice point of the smallest lattice edge / face / cell that holds vertex v (index
//   units) is observed (count >= min_count): a marching-cubes vertex has one fractional coordinate -> the two ends of its edge;
//   none -> that one lattice point.  A vertex outside the lattice (or NaN) is not kept.
// mesh filter (Open3D's remove_vertices_by_mask, keep = 1 means stay), integers only, the passes of mesh.hip:
//   k_mf_count      per workgroup of 256 indices: kept vertices and kept triangles (all three corners in [0, V) and kept)
//   k_mf_scan       ONE workgroup: exclusive scans of both totals (scan.h workgroup_scan) -> counts[4] = Vk, Tk, 0, 0
//   k_mf_vertices   new index of every vertex (workspace) and the kept vertices, in order
//   k_mf_triangles  the kept triangles, in order, renumbered
// Workspace: vertex totals u32[Gv] | triangle totals u32[Gt] | vertex offsets u32[Gv] | triangle offsets u32[Gt] | new index
// u32[V]; Gv = ceil(V / 256), Gt = ceil(T / 256).
#include <cmath>

#include "common.h"
#include "pano_geom.h"
#include "scan.h"

namespace {

constexpr uint32_t kTsdfThreads = 256;
constexpr uint32_t kBrick = 4;            // lattice points per brick edge: 4^3 = one wave
constexpr uint32_t kBricksPerGroup = 4;   // bricks of a workgroup, stacked in z
static_assert(kBrick * kBrick * kBrick == LNH_WAVE && kBricksPerGroup * LNH_WAVE == kTsdfThreads, "a brick is a wave");
constexpr float kTsdfFill = 1.0f;
constexpr uint64_t kTsdfMaxPixels = 1ull << 24;

__host__ __device__ __forceinline__ uint32_t div_up_dev(uint32_t a, uint32_t b) { return (a + b - 1) / b; }  // a + b < 2^32 here

struct TsdfLattice {
    float lo[3], step[3];
    uint32_t nx, ny, nz, n;  // n = nx * ny * nz < 2^31
};

__global__ void __launch_bounds__(kTsdfThreads)
k_tsdf_integrate(const float *__restrict__ panos, const float *__restrict__ w2l, uint32_t F, PanoGeom g, TsdfLattice L,
                 float trunc, float *__restrict__ sum, uint32_t *__restrict__ count) {
    // workgroup b of the 1-D grid = brick column (bx, by, bz), z fastest
    const uint32_t gz = div_up_dev(L.nz, kBrick * kBricksPerGroup), gy = div_up_dev(L.ny, kBrick);
    const uint32_t bz = blockIdx.x % gz, bxy = blockIdx.x / gz, by = bxy % gy, bx = bxy / gy;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t ix = bx * kBrick + (lane >> 4), iy = by * kBrick + ((lane >> 2) & 3),
                   iz = (bz * kBricksPerGroup + wv) * kBrick + (lane & 3);
    if (ix >= L.nx || iy >= L.ny || iz >= L.nz) return;
    const uint32_t p = (ix * L.ny + iy) * L.nz + iz;  // < n
    const float px = L.lo[0] + (float)ix * L.step[0], py = L.lo[1] + (float)iy * L.step[1], pz = L.lo[2] + (float)iz * L.step[2];
    const size_t HW = (size_t)g.H * g.W;
    float s = sum[p];
    uint32_t c = count[p];
    for (uint32_t f = 0; f < F; f++) {
        const float *__restrict__ m = w2l + (size_t)f * 12;  // uniform over the wave: scalar loads
        const float qx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
        const float qy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
        const float qz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
        float r;
        const uint32_t pix = pano_pixel_xyz<true>(qx, qy, qz, g, r);  // (tests r against max_depth before the two atan2)
        if (pix == kNoPixel) continue;
        const float d = panos[f * HW + pix];  // pix < H * W
        if (!(d > 0.0f) || !(d < INFINITY)) continue;
        const float sd = d - r;
        if (sd < -trunc) continue;
        s += fminf(sd / trunc, 1.0f);
        c += 1u;
    }
    sum[p] = s;
    count[p] = c;
}

__global__ void __launch_bounds__(256)
k_tsdf_finalize(const float *__restrict__ sum, const uint32_t *__restrict__ count, uint32_t n, uint32_t min_count,
                float *__restrict__ volume) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t c = count[p];
    volume[p] = c >= min_count ? -(sum[p] / (float)c) : kTsdfFill;  // (min_count >= 1: no division by 0)
}

__global__ void __launch_bounds__(256)
k_mesh_vertex_observed(const float *__restrict__ vertices, uint32_t V, const uint32_t *__restrict__ count, uint32_t nx, uint32_t ny,
                       uint32_t nz, uint32_t min_count, uint8_t *__restrict__ keep) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const uint32_t dims[3] = {nx, ny, nz}, strides[3] = {ny * nz, nz, 1u};
    uint32_t base = 0, far[3];
    bool inside = true;
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) {
        // inside [0, n - 1], compared in integers behind the floor (float(n - 1) is not exact above 2^24)
        const float x = vertices[(size_t)v * 3 + a];
        const bool finite_index = x >= 0.0f && x < 2147483648.0f;  // (a NaN fails)
        const float fl = floorf(finite_index ? x : 0.0f);
        const uint32_t i = (uint32_t)fl, frac = (finite_index && x != fl) ? 1u : 0u;
        const bool ok = finite_index && i + frac <= dims[a] - 1;  // a fractional coordinate needs its far end i + 1
        inside = inside && ok;
        base += (ok ? i : 0u) * strides[a];
        far[a] = (ok && frac) ? strides[a] : 0u;
    }
    bool observed = inside;
    if (inside) {
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t q = base + (k & 1) * far[0] + ((k >> 1) & 1) * far[1] + (k >> 2) * far[2];  // < nx * ny * nz
            observed = observed && count[q] >= min_count;
        }
    }
    keep[v] = observed ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------- mesh filter
__device__ __forceinline__ bool mf_triangle_kept(const uint8_t *__restrict__ keep, uint32_t V, const int32_t *__restrict__ tri,
                                                 uint32_t t, uint32_t &a, uint32_t &b, uint32_t &c) {
    a = (uint32_t)tri[(size_t)t * 3], b = (uint32_t)tri[(size_t)t * 3 + 1], c = (uint32_t)tri[(size_t)t * 3 + 2];
    if (a >= V || b >= V || c >= V) return false;  // (a negative index is a large unsigned one)
    return keep[a] && keep[b] && keep[c];
}

constexpr uint32_t kMfTriShift = 16;  // kept vertices (<= 256) in bits 0-15, kept triangles (<= 256) above

__global__ void __launch_bounds__(256)
k_mf_count(const uint8_t *__restrict__ keep, uint32_t V, const int32_t *__restrict__ tri, uint32_t T, uint32_t Gv, uint32_t Gt,
           uint32_t *__restrict__ vtot, uint32_t *__restrict__ ttot) {
    __shared__ uint32_t s_wave[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t a, b, c;
    const uint32_t kv = (i < V && keep[i]) ? 1u : 0u, kt = (i < T && mf_triangle_kept(keep, V, tri, i, a, b, c)) ? 1u : 0u;
    uint32_t total;
    (void)block_scan_256(kv | kt << kMfTriShift, s_wave, total);
    if (threadIdx.x == 0) {
        if (blockIdx.x < Gv) vtot[blockIdx.x] = total & ((1u << kMfTriShift) - 1);
        if (blockIdx.x < Gt) ttot[blockIdx.x] = total >> kMfTriShift;
    }
}

__global__ void __launch_bounds__(kScanThreads)
k_mf_scan(const uint32_t *__restrict__ vtot, uint32_t Gv, const uint32_t *__restrict__ ttot, uint32_t Gt, uint32_t *__restrict__ voff,
          uint32_t *__restrict__ toff, uint32_t *__restrict__ counts) {
    // (V, T < 2^31: both totals fit 32 bits)
    const uint32_t nv = workgroup_scan<uint32_t>(
        Gv, 0u, [&](uint32_t g, bool) { return vtot[g]; }, [&](uint32_t g, uint32_t off) { voff[g] = off; });
    const uint32_t nt = workgroup_scan<uint32_t>(
        Gt, 0u, [&](uint32_t g, bool) { return ttot[g]; }, [&](uint32_t g, uint32_t off) { toff[g] = off; });
    if (threadIdx.x == 0) counts[0] = nv, counts[1] = nt, counts[2] = 0u, counts[3] = 0u;
}

__global__ void __launch_bounds__(256)
k_mf_vertices(const float *__restrict__ vertices, const uint8_t *__restrict__ keep, uint32_t V, const uint32_t *__restrict__ voff,
              uint32_t *__restrict__ vmap, float *__restrict__ out, uint32_t max_vertices) {
    __shared__ uint32_t s_wave[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t kv = (i < V && keep[i]) ? 1u : 0u;
    uint32_t total;
    const uint32_t k = voff[blockIdx.x] + block_scan_256(kv, s_wave, total);
    if (i >= V) return;
    vmap[i] = k;
    if (!kv || k >= max_vertices) return;
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) out[(size_t)k * 3 + a] = vertices[(size_t)i * 3 + a];
}

__global__ void __launch_bounds__(256)
k_mf_triangles(const uint8_t *__restrict__ keep, uint32_t V, const int32_t *__restrict__ tri, uint32_t T,
               const uint32_t *__restrict__ toff, const uint32_t *__restrict__ vmap, int32_t *__restrict__ out,
               uint32_t max_triangles) {
    __shared__ uint32_t s_wave[4];
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    uint32_t a = 0, b = 0, c = 0;
    const uint32_t kt = (t < T && mf_triangle_kept(keep, V, tri, t, a, b, c)) ? 1u : 0u;
    uint32_t total;
    const uint32_t k = toff[blockIdx.x] + block_scan_256(kt, s_wave, total);
    if (!kt || k >= max_triangles) return;
    int32_t *o = out + (size_t)k * 3;
    o[0] = (int32_t)vmap[a], o[1] = (int32_t)vmap[b], o[2] = (int32_t)vmap[c];  // (a, b, c < V: kept)
}

struct MfLayout {
    uint64_t vtot, ttot, voff, toff, vmap, bytes;
    uint32_t gv, gt;
};
MfLayout mf_layout(uint64_t V, uint64_t T) {
    MfLayout l;
    l.gv = div_up(V, 256), l.gt = div_up(T, 256);
    l.vtot = 0;
    l.ttot = l.vtot + 4ull * l.gv;
    l.voff = l.ttot + 4ull * l.gt;
    l.toff = l.voff + 4ull * l.gv;
    l.vmap = l.toff + 4ull * l.gt;
    l.bytes = (l.vmap + 4ull * V + 15) & ~15ull;
    return l;
}
bool mf_sizes_ok(uint32_t V, uint32_t T) { return V >= 1 && T >= 1 && V < (1u << 31) && T < (1u << 31); }

bool tsdf_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const uint64_t xy = (uint64_t)nx * ny;
    return xy < (1ull << 31) && xy * nz < (1ull << 31);
}
int tsdf_dims_check(const char *who, uint32_t nx, uint32_t ny, uint32_t nz) {
    LNH_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, LNH_ERR_INVALID_ARG, "%s: lattice of %u x %u x %u points, every dimension must be >= 2",
                who, nx, ny, nz);
    LNH_REQUIRE(tsdf_dims_ok(nx, ny, nz), LNH_ERR_UNSUPPORTED, "%s: %u x %u x %u points, point indices are 31 bits wide (nx*ny*nz < 2^31)",
                who, nx, ny, nz);
    return LNH_OK;
}

int mf_check(const char *who, const uint8_t *keep, uint32_t V, const int32_t *triangles, uint32_t T, const void *ws,
             uint64_t ws_bytes) {
    LNH_REQUIRE(keep && triangles && ws, LNH_ERR_INVALID_ARG, "%s: null pointer", who);
    LNH_REQUIRE(V >= 1 && T >= 1, LNH_ERR_INVALID_ARG, "%s: %u vertices and %u triangles: an empty mesh needs no call", who, V, T);
    LNH_REQUIRE(mf_sizes_ok(V, T), LNH_ERR_UNSUPPORTED, "%s: %u vertices and %u triangles, indices are int32 (fewer than 2^31)", who,
                V, T);
    const MfLayout l = mf_layout(V, T);
    LNH_REQUIRE(((uintptr_t)ws & 3) == 0 && ws_bytes >= l.bytes, LNH_ERR_INVALID_ARG,
                "%s: workspace of %llu bytes (4-byte aligned) needed, got %llu", who, (unsigned long long)l.bytes,
                (unsigned long long)ws_bytes);
    return LNH_OK;
}

}  // namespace

extern "C" {

int lnh_tsdf_integrate(const float *panos, const float *world_to_lidar, uint32_t F, uint32_t H, uint32_t W, float fov_up, float fov,
                       float max_depth, const float *lo, const float *step, uint32_t nx, uint32_t ny, uint32_t nz, float trunc,
                       float *sum, uint32_t *count, lnh_stream_t stream) {
    LNH_REQUIRE(panos && world_to_lidar && lo && step && sum && count, LNH_ERR_INVALID_ARG, "tsdf_integrate: null pointer");
    LNH_REQUIRE(F >= 1 && H >= 1 && W >= 1, LNH_ERR_INVALID_ARG, "tsdf_integrate: %u frames of %u x %u pixels: none may be 0", F, H, W);
    LNH_REQUIRE((uint64_t)H * W <= kTsdfMaxPixels, LNH_ERR_UNSUPPORTED, "tsdf_integrate: H * W = %llu, at most 2^24 pixels",
                (unsigned long long)H * W);
    int rc = tsdf_dims_check("tsdf_integrate", nx, ny, nz);
    if (rc) return rc;
    LNH_REQUIRE(fov > 0.0f, LNH_ERR_INVALID_ARG, "tsdf_integrate: fov must be positive");
    LNH_REQUIRE(trunc > 0.0f && trunc < INFINITY, LNH_ERR_INVALID_ARG, "tsdf_integrate: trunc must be positive and finite");
    TsdfLattice L;
    for (int a = 0; a < 3; a++) {
        LNH_REQUIRE(step[a] > 0.0f && step[a] < INFINITY, LNH_ERR_INVALID_ARG, "tsdf_integrate: step[%d] must be positive and finite", a);
        LNH_REQUIRE(std::isfinite(lo[a]), LNH_ERR_INVALID_ARG, "tsdf_integrate: lo[%d] is not finite", a);
        L.lo[a] = lo[a], L.step[a] = step[a];
    }
    L.nx = nx, L.ny = ny, L.nz = nz, L.n = nx * ny * nz;
    const PanoGeom g = pano_geom(H, W, fov_up, fov, max_depth);
    hipStream_t s = (hipStream_t)stream;
    // (every factor is at most its dimension, so the number of workgroups stays below nx * ny * nz < 2^31)
    const uint64_t groups = (uint64_t)div_up(nx, kBrick) * div_up(ny, kBrick) * div_up(nz, kBrick * kBricksPerGroup);
    LNH_LAUNCH(k_tsdf_integrate, dim3((uint32_t)groups), dim3(kTsdfThreads), 0, s, panos, world_to_lidar, F, g, L, trunc, sum, count);
    return lnh_check_launch("lnh_tsdf_integrate");
}

int lnh_tsdf_finalize(const float *sum, const uint32_t *count, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t min_count,
                      float *volume, lnh_stream_t stream) {
    LNH_REQUIRE(sum && count && volume, LNH_ERR_INVALID_ARG, "tsdf_finalize: null pointer");
    int rc = tsdf_dims_check("tsdf_finalize", nx, ny, nz);
    if (rc) return rc;
    LNH_REQUIRE(min_count >= 1, LNH_ERR_INVALID_ARG, "tsdf_finalize: min_count must be at least 1");
    const uint32_t n = nx * ny * nz;
    LNH_LAUNCH(k_tsdf_finalize, dim3(div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, sum, count, n, min_count, volume);
    return lnh_check_launch("lnh_tsdf_finalize");
}

int lnh_mesh_vertex_observed(const float *vertices, uint32_t V, const uint32_t *count, uint32_t nx, uint32_t ny, uint32_t nz,
                             uint32_t min_count, uint8_t *keep, lnh_stream_t stream) {
    LNH_REQUIRE(vertices && count && keep, LNH_ERR_INVALID_ARG, "mesh_vertex_observed: null pointer");
    LNH_REQUIRE(V >= 1, LNH_ERR_INVALID_ARG, "mesh_vertex_observed: no vertices: an empty mesh needs no call");
    LNH_REQUIRE(V < (1u << 31), LNH_ERR_UNSUPPORTED, "mesh_vertex_observed: V = %u, indices are int32 (fewer than 2^31)", V);
    int rc = tsdf_dims_check("mesh_vertex_observed", nx, ny, nz);
    if (rc) return rc;
    LNH_REQUIRE(min_count >= 1, LNH_ERR_INVALID_ARG, "mesh_vertex_observed: min_count must be at least 1");
    LNH_LAUNCH(k_mesh_vertex_observed, dim3(div_up(V, 256)), dim3(256), 0, (hipStream_t)stream, vertices, V, count, nx, ny, nz,
               min_count, keep);
    return lnh_check_launch("lnh_mesh_vertex_observed");
}

uint64_t lnh_mesh_filter_workspace_size(uint32_t V, uint32_t T) {
    if (!mf_sizes_ok(V, T)) return 0;
    return mf_layout(V, T).bytes;
}

int lnh_mesh_filter_count(const uint8_t *keep, uint32_t V, const int32_t *triangles, uint32_t T, void *ws, uint64_t ws_bytes,
                          uint32_t *counts, lnh_stream_t stream) {
    int rc = mf_check("mesh_filter_count", keep, V, triangles, T, ws, ws_bytes);
    if (rc) return rc;
    LNH_REQUIRE(counts && ((uintptr_t)counts & 3) == 0, LNH_ERR_INVALID_ARG, "mesh_filter_count: null pointer (counts)");
    const MfLayout l = mf_layout(V, T);
    char *w = (char *)ws;
    uint32_t *vtot = (uint32_t *)(w + l.vtot), *ttot = (uint32_t *)(w + l.ttot), *voff = (uint32_t *)(w + l.voff),
             *toff = (uint32_t *)(w + l.toff);
    hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_mf_count, dim3(l.gv > l.gt ? l.gv : l.gt), dim3(256), 0, s, keep, V, triangles, T, l.gv, l.gt, vtot, ttot);
    if ((rc = lnh_check_launch("lnh_mesh_filter_count(count)"))) return rc;
    LNH_LAUNCH(k_mf_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)vtot, l.gv, (const uint32_t *)ttot, l.gt, voff, toff,
               counts);
    return lnh_check_launch("lnh_mesh_filter_count(scan)");
}

int lnh_mesh_filter_emit(const float *vertices, const uint8_t *keep, uint32_t V, const int32_t *triangles, uint32_t T, void *ws,
                         uint64_t ws_bytes, float *out_vertices, uint32_t max_vertices, int32_t *out_triangles,
                         uint32_t max_triangles, lnh_stream_t stream) {
    int rc = mf_check("mesh_filter_emit", keep, V, triangles, T, ws, ws_bytes);
    if (rc) return rc;
    LNH_REQUIRE(vertices && out_vertices, LNH_ERR_INVALID_ARG, "mesh_filter_emit: null pointer (vertices)");
    LNH_REQUIRE(max_vertices >= 1, LNH_ERR_INVALID_ARG, "mesh_filter_emit: capacity of 0 vertices: an empty mesh needs no call");
    LNH_REQUIRE(out_triangles || max_triangles == 0, LNH_ERR_INVALID_ARG, "mesh_filter_emit: null pointer (triangles)");
    const MfLayout l = mf_layout(V, T);
    char *w = (char *)ws;
    const uint32_t *voff = (const uint32_t *)(w + l.voff), *toff = (const uint32_t *)(w + l.toff);
    uint32_t *vmap = (uint32_t *)(w + l.vmap);
    hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_mf_vertices, dim3(l.gv), dim3(256), 0, s, vertices, keep, V, voff, vmap, out_vertices, max_vertices);
    if ((rc = lnh_check_launch("lnh_mesh_filter_emit(vertices)"))) return rc;
    if (max_triangles == 0) return LNH_OK;  // (every triangle touched a removed vertex: the vertices alone)
    LNH_LAUNCH(k_mf_triangles, dim3(l.gt), dim3(256), 0, s, keep, V, triangles, T, toff, (const uint32_t *)vmap, out_triangles,
               max_triangles);
    return lnh_check_launch("lnh_mesh_filter_emit(triangles)");
}

}  // extern "C"
