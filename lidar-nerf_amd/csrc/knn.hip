// knn.hip — exact k-nearest neighbours of a point cloud on the GPU over a uniform grid: what lidarnvs/lidarnvs_meshing.py does in
// predict_frame with Open3D's KDTreeFlann.search_knn_vector_3d (one Python iteration per hit point) and np.mean of the
// neighbours' intensities.
//
// THE DISTANCE of a point p from a query q, fp32, the library is built with -ffp-contract=off, one rounded operation per operator:
//   dx = p.x - q.x      dy = p.y - q.y      dz = p.z - q.z      d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
// d2 >= 0 (never NaN for finite operands: a square is not negative, so nothing cancels), its bit pattern orders like its value.
//
// THE ANSWER FOR A QUERY is the min(k, N) smallest 64-bit keys (bits of d2) << 32 | point index over ALL points, in ascending
// order: nearest first, among equal distances the smallest index.  1 <= k <= 16.
//
// THE GRID only decides when the walk may stop (DESIGN §16 has the argument).  Box = exact min / max of the points; extent
// e[a] = max(hi[a] - lo[a], largest extent * 2^-10) (1 when the cloud is one point), cell_of(x) = clamp(floorf((x - lo[a]) *
// (n[a] / e[a])), 0, n[a] - 1): monotone in x, shared by the build and the search (a query outside the box is clamped into it).
// The build records per axis a and slab i the smallest and largest coordinate of the points whose cell index along a is i, and
// from them smin[a][i] = min over the slabs >= i, pmax[a][i] = max over the slabs <= i (+inf / -inf where there is no point).
// The search visits the shells r = 0, 1, 2, ... of cells around the query's cell c (Chebyshev distance r) and tests every point
// of a shell before it looks at the stopping test: stop when the block [c - r, c + r] covers the grid, or when k keys are held
// and d2 of the k-th < g * g (strictly: an untested point at an equal distance could still win on its index), with
//   g = min over the axes of max(smin[a][c_a + r + 1] - q_a, 0) and max(q_a - pmax[a][c_a - r - 1], 0), where that slab exists.
// A column (x, y) or a cell of a shell is skipped when the same kind of lower bound already exceeds the k-th key: the points
// skipped could not have entered.  A grid of 1 x 1 x 1 reads the point array itself.
//
// The grid itself (box -> cells, cell_of, the bounds passes' reduce) is cell_grid.h, shared with raycast.hip; the scan is scan.h.
// Build passes, none waits for another workgroup: k_knn_bounds (per-workgroup min / max / count, no atomics), k_knn_bounds_finish
// (one workgroup), k_knn_count (integer atomics: a counter per cell, min / max per slab on an order-preserving integer encoding
// of the float), k_knn_scan (one workgroup, scan.h workgroup_scan; its first threads also form smin / pmax), k_knn_fill (an
// integer cursor per cell: the order inside a cell is arrival order and no output depends on it).  The fill writes the points
// sorted by cell as 16-byte rows (x, y, z, bits of the original index): the cells (x, y, z0 ... z1) are ONE contiguous read.
#include "common.h"
#include "knn_walk.h"
#include "scan.h"

namespace {

constexpr uint32_t kKnnThreads = kCellThreads;
constexpr uint32_t kKnnBoundsWords = 8;  // per-workgroup partial (cell_grid.h): lo[3], hi[3], non-finite coordinates, 0
constexpr uint32_t kKnnSearchThreads = 128;
constexpr uint32_t kKnnMaxK = 16;

// float -> unsigned, order-preserving (for the integer atomicMin / atomicMax of the slab extremes), and back
__device__ __forceinline__ uint32_t knn_enc(float x) {
    const uint32_t b = __float_as_uint(x);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float knn_dec(uint32_t e) { return __uint_as_float(e & 0x80000000u ? e & 0x7fffffffu : ~e); }

// --------------------------------------------------------------------------------------------------------------- bounds
__global__ void __launch_bounds__(kKnnThreads)
k_knn_bounds(const float *__restrict__ points, uint32_t N, uint32_t *__restrict__ partials) {
    const float inf = __uint_as_float(0x7f800000u);
    float f[6] = {inf, inf, inf, -inf, -inf, -inf};
    uint32_t bad[1] = {0};
    cell_bounds_accumulate(points, N, f, f + 3, bad[0]);
    cell_block_reduce(f, bad, partials + (size_t)blockIdx.x * kKnnBoundsWords);
}

__global__ void __launch_bounds__(kKnnThreads)
k_knn_bounds_finish(const uint32_t *__restrict__ partials, uint32_t G, uint32_t *__restrict__ box) {
    const float inf = __uint_as_float(0x7f800000u);
    float f[6] = {inf, inf, inf, -inf, -inf, -inf};
    uint32_t bad[1] = {0};
    cell_merge_partials(partials, G, f, bad);
    __shared__ uint32_t s_out[kKnnBoundsWords];
    cell_block_reduce(f, bad, s_out);
    __syncthreads();
    if (threadIdx.x < kKnnBoundsWords) box[threadIdx.x] = s_out[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------- the cells
struct KnnCell {
    uint32_t c[3];
    float p[3];
};
__device__ __forceinline__ KnnCell knn_point_cell(const float *__restrict__ points, uint32_t i, const CellGrid &g) {
    KnnCell k;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        k.p[a] = points[(size_t)i * 3 + a];
        k.c[a] = cell_of(k.p[a], g.lo[a], g.inv[a], g.n[a]);
    }
    return k;
}

// slab_enc: u32 [2][nx + ny + nz], the smallest and the largest encoded coordinate per slab (preset to ~0 and 0)
__global__ void __launch_bounds__(kKnnThreads)
k_knn_count(const float *__restrict__ points, uint32_t N, const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz,
            uint32_t *__restrict__ cell_count, uint32_t *__restrict__ slab_enc) {
    const uint32_t i = blockIdx.x * kKnnThreads + threadIdx.x;
    if (i >= N) return;
    const CellGrid g = cell_grid(box, nx, ny, nz);
    const KnnCell k = knn_point_cell(points, i, g);
    atomicAdd(&cell_count[(k.c[0] * ny + k.c[1]) * nz + k.c[2]], 1u);  // < cells
    const uint32_t S = nx + ny + nz, off[3] = {0u, nx, nx + ny};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const uint32_t e = knn_enc(k.p[a]), s = off[a] + k.c[a];  // < S
        // an extreme only moves one way: a value read earlier can only ask for an atomic that was not needed
        if (e < __hip_atomic_load(&slab_enc[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&slab_enc[s], e);
        if (e > __hip_atomic_load(&slab_enc[S + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&slab_enc[S + s], e);
    }
}

__global__ void __launch_bounds__(kKnnThreads)
k_knn_slab_preset(uint32_t *__restrict__ slab_enc, uint32_t S) {
    const uint32_t i = blockIdx.x * kKnnThreads + threadIdx.x;
    if (i < S) slab_enc[i] = 0xffffffffu;
    else if (i < 2 * S) slab_enc[i] = 0u;
}

// exclusive scan of cell_count[cells] -> cell_start[cells + 1]; threads 0 ... 5 also turn the slab extremes into
// slabs f32 [2][nx + ny + nz]: smin (minimum over the slabs >= i) and pmax (maximum over the slabs <= i) per axis
__global__ void __launch_bounds__(kScanThreads)
k_knn_scan(const uint32_t *__restrict__ cell_count, uint32_t cells, uint32_t *__restrict__ cell_start,
           const uint32_t *__restrict__ slab_enc, uint32_t nx, uint32_t ny, uint32_t nz, float *__restrict__ slabs) {
    if (threadIdx.x < 6) {
        const uint32_t a = threadIdx.x % 3, S = nx + ny + nz;
        const uint32_t n = a == 0 ? nx : (a == 1 ? ny : nz), off = a == 0 ? 0u : (a == 1 ? nx : nx + ny);
        if (threadIdx.x < 3) {
            float m = __uint_as_float(0x7f800000u);
            for (uint32_t i = n; i-- > 0;) {
                const uint32_t e = slab_enc[off + i];
                if (e != 0xffffffffu) m = fminf(m, knn_dec(e));  // (an empty slab keeps its preset)
                slabs[off + i] = m;
            }
        } else {
            float m = __uint_as_float(0xff800000u);
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t e = slab_enc[S + off + i];
                if (e != 0u) m = fmaxf(m, knn_dec(e));
                slabs[S + off + i] = m;
            }
        }
    }
    const uint32_t total = workgroup_scan<uint32_t>(  // (the total is N < 2^31)
        cells, 0u, [&](uint32_t c, bool) { return cell_count[c]; }, [&](uint32_t c, uint32_t at) { cell_start[c] = at; });
    if (threadIdx.x == 0) cell_start[cells] = total;
}

__global__ void __launch_bounds__(kKnnThreads)
k_knn_fill(const float *__restrict__ points, uint32_t N, const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz,
           const uint32_t *__restrict__ cell_start, uint32_t *__restrict__ cursor, float4_t *__restrict__ sorted) {
    const uint32_t i = blockIdx.x * kKnnThreads + threadIdx.x;
    if (i >= N) return;
    const CellGrid g = cell_grid(box, nx, ny, nz);
    const KnnCell k = knn_point_cell(points, i, g);
    const uint32_t c = (k.c[0] * ny + k.c[1]) * nz + k.c[2];
    const uint32_t slot = cell_start[c] + atomicAdd(&cursor[c], 1u);
    if (slot < cell_start[c + 1] && slot < N) {  // (never outside the buffer)
        float4_t row;
        row.x = k.p[0], row.y = k.p[1], row.z = k.p[2], row.w = __uint_as_float(i);
        sorted[slot] = row;
    }
}

// ----------------------------------------------------------------------------------------------------------- the search
// (knn_walk.h has the walk of one query: KnnBest, knn_key, knn_walk)
template <int K>
__global__ void __launch_bounds__(kKnnSearchThreads)
k_knn_search(KnnArgs A) {
    const uint32_t qi = blockIdx.x * kKnnSearchThreads + threadIdx.x;
    if (qi >= A.Q) return;
    const float inf = __uint_as_float(0x7f800000u);
    const float q[3] = {A.queries[(size_t)qi * 3], A.queries[(size_t)qi * 3 + 1], A.queries[(size_t)qi * 3 + 2]};
    const uint32_t k = A.k, N = A.N;
    KnnBest<K> best;
    best.clear(k);
    const bool live = (!A.valid || A.valid[qi] != 0) && cell_finite(q[0]) && cell_finite(q[1]) && cell_finite(q[2]);
    if (live) knn_walk<K>(A, q, best);
    double sum = 0.0;
    uint32_t held = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const uint32_t rank = (uint32_t)j + k - (uint32_t)K;  // slot j holds rank j - (K - k)
        if ((uint32_t)j + k >= (uint32_t)K) {
            const unsigned long long key = best.key[j];
            const bool has = key != ~0ull;
            const uint32_t index = min((uint32_t)key - 1u, N - 1);
            if (A.indices) A.indices[(size_t)qi * k + rank] = has ? (int32_t)index : -1;
            if (A.dist2) A.dist2[(size_t)qi * k + rank] = has ? __uint_as_float((uint32_t)(key >> 32)) : inf;
            if (A.values && has) sum += (double)A.values[index], held++;
        }
    }
    if (A.mean) A.mean[qi] = held ? (float)(sum / (double)held) : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------ host side
// workspace: the cell counters u32[cells], then the slab extremes u32[2][nx + ny + nz]; the bounds partials overlay them
uint64_t knn_ws_bytes(uint32_t N, uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint64_t bounds = 4ull * kKnnBoundsWords * cell_bounds_groups(N);
    const uint64_t cells = 4ull * nx * ny * nz + 8ull * ((uint64_t)nx + ny + nz);
    return ((bounds > cells ? bounds : cells) + 15) & ~15ull;
}
int knn_check_cloud(const char *who, const float *points, uint32_t N) {
    LNH_REQUIRE(points && ((uintptr_t)points & 3) == 0, LNH_ERR_INVALID_ARG, "%s: null pointer (points)", who);
    LNH_REQUIRE(N >= 1, LNH_ERR_INVALID_ARG, "%s: empty cloud (0 points)", who);
    LNH_REQUIRE(N < (1u << 31), LNH_ERR_UNSUPPORTED, "%s: %u points, indices are int32 (< 2^31)", who, N);
    return LNH_OK;
}
int knn_check_ws(const char *who, uint32_t N, uint32_t nx, uint32_t ny, uint32_t nz, const void *ws, uint64_t ws_bytes) {
    return cell_check_ws(who, knn_ws_bytes(N, nx, ny, nz), ws, ws_bytes);
}

template <int K>
void knn_launch(const KnnArgs &A, hipStream_t s) {
    LNH_LAUNCH(k_knn_search<K>, dim3(div_up(A.Q, kKnnSearchThreads)), dim3(kKnnSearchThreads), 0, s, A);
}

}  // namespace

extern "C" {

uint64_t lnh_knn_workspace_size(uint32_t N, uint32_t nx, uint32_t ny, uint32_t nz) {
    if (N < 1 || N >= (1u << 31) || !cell_grid_ok(nx, ny, nz)) return 0;
    return knn_ws_bytes(N, nx, ny, nz);
}

int lnh_knn_bounds(const float *points, uint32_t N, void *ws, uint64_t ws_bytes, float *box, lnh_stream_t stream) {
    int rc = knn_check_cloud("knn_bounds", points, N);
    if (rc) return rc;
    LNH_REQUIRE(box && ((uintptr_t)box & 3) == 0, LNH_ERR_INVALID_ARG, "knn_bounds: null pointer (box)");
    if ((rc = knn_check_ws("knn_bounds", N, 1, 1, 1, ws, ws_bytes))) return rc;
    const uint32_t G = cell_bounds_groups(N);
    hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_knn_bounds, dim3(G), dim3(kKnnThreads), 0, s, points, N, (uint32_t *)ws);
    if ((rc = lnh_check_launch("lnh_knn_bounds(partials)"))) return rc;
    LNH_LAUNCH(k_knn_bounds_finish, dim3(1), dim3(kKnnThreads), 0, s, (const uint32_t *)ws, G, (uint32_t *)box);
    return lnh_check_launch("lnh_knn_bounds(finish)");
}

int lnh_knn_build_count(const float *points, uint32_t N, const float *box, uint32_t nx, uint32_t ny, uint32_t nz, void *ws,
                        uint64_t ws_bytes, uint32_t *cell_start, float *slabs, lnh_stream_t stream) {
    int rc = knn_check_cloud("knn_build_count", points, N);
    if (rc) return rc;
    if ((rc = cell_check_grid("knn_build_count", box, nx, ny, nz))) return rc;
    LNH_REQUIRE(cell_start && slabs && ((uintptr_t)cell_start & 3) == 0 && ((uintptr_t)slabs & 3) == 0, LNH_ERR_INVALID_ARG,
                "knn_build_count: null pointer (cell_start / slabs)");
    if ((rc = knn_check_ws("knn_build_count", N, nx, ny, nz, ws, ws_bytes))) return rc;
    const uint32_t cells = nx * ny * nz, S = nx + ny + nz;  // cells <= 2^30
    uint32_t *cell_count = (uint32_t *)ws, *slab_enc = cell_count + cells;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lnh_zero_async(ws, 4ull * cells, s, "lnh_knn_build_count(clear)"))) return rc;
    LNH_LAUNCH(k_knn_slab_preset, dim3(div_up(2 * S, kKnnThreads)), dim3(kKnnThreads), 0, s, slab_enc, S);
    if ((rc = lnh_check_launch("lnh_knn_build_count(preset)"))) return rc;
    LNH_LAUNCH(k_knn_count, dim3(div_up(N, kKnnThreads)), dim3(kKnnThreads), 0, s, points, N, box, nx, ny, nz, cell_count, slab_enc);
    if ((rc = lnh_check_launch("lnh_knn_build_count(count)"))) return rc;
    LNH_LAUNCH(k_knn_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)cell_count, cells, cell_start,
               (const uint32_t *)slab_enc, nx, ny, nz, slabs);
    return lnh_check_launch("lnh_knn_build_count(scan)");
}

int lnh_knn_build_fill(const float *points, uint32_t N, const float *box, uint32_t nx, uint32_t ny, uint32_t nz, void *ws,
                       uint64_t ws_bytes, const uint32_t *cell_start, float *sorted, lnh_stream_t stream) {
    int rc = knn_check_cloud("knn_build_fill", points, N);
    if (rc) return rc;
    if ((rc = cell_check_grid("knn_build_fill", box, nx, ny, nz))) return rc;
    LNH_REQUIRE(cell_start && sorted && ((uintptr_t)cell_start & 3) == 0, LNH_ERR_INVALID_ARG,
                "knn_build_fill: null pointer (cell_start / sorted)");
    LNH_REQUIRE(((uintptr_t)sorted & 15) == 0, LNH_ERR_INVALID_ARG, "knn_build_fill: sorted must be 16-byte aligned (rows of 16 bytes)");
    if ((rc = knn_check_ws("knn_build_fill", N, nx, ny, nz, ws, ws_bytes))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lnh_zero_async(ws, 4ull * nx * ny * nz, s, "lnh_knn_build_fill(clear)"))) return rc;
    LNH_LAUNCH(k_knn_fill, dim3(div_up(N, kKnnThreads)), dim3(kKnnThreads), 0, s, points, N, box, nx, ny, nz, cell_start, (uint32_t *)ws,
               (float4_t *)sorted);
    return lnh_check_launch("lnh_knn_build_fill");
}

int lnh_knn_search(const float *points, uint32_t N, const float *box, uint32_t nx, uint32_t ny, uint32_t nz,
                   const uint32_t *cell_start, const float *sorted, const float *slabs, const float *queries, const uint8_t *valid,
                   uint32_t Q, uint32_t k, const float *values, int32_t *indices, float *dist2, float *mean, lnh_stream_t stream) {
    int rc = knn_check_cloud("knn_search", points, N);
    if (rc) return rc;
    if ((rc = cell_check_grid("knn_search", box, nx, ny, nz))) return rc;
    LNH_REQUIRE(cell_start && sorted && slabs && ((uintptr_t)cell_start & 3) == 0 && ((uintptr_t)slabs & 3) == 0, LNH_ERR_INVALID_ARG,
                "knn_search: null pointer (cell_start / sorted / slabs)");
    LNH_REQUIRE(((uintptr_t)sorted & 15) == 0, LNH_ERR_INVALID_ARG, "knn_search: sorted must be 16-byte aligned (rows of 16 bytes)");
    LNH_REQUIRE(k >= 1 && k <= kKnnMaxK, LNH_ERR_INVALID_ARG, "knn_search: k = %u, must be 1 ... %u", k, kKnnMaxK);
    LNH_REQUIRE((values != nullptr) == (mean != nullptr), LNH_ERR_INVALID_ARG,
                "knn_search: values and mean go together (both or neither)");
    LNH_REQUIRE(indices || dist2 || mean, LNH_ERR_INVALID_ARG, "knn_search: no output (indices / dist2 / mean are all null)");
    if (Q == 0) return LNH_OK;
    LNH_REQUIRE(Q < (1u << 31), LNH_ERR_UNSUPPORTED, "knn_search: %u queries, at most 2^31 - 1 per call", Q);
    LNH_REQUIRE(queries && ((uintptr_t)queries & 3) == 0, LNH_ERR_INVALID_ARG, "knn_search: null pointer (queries)");
    const KnnArgs A = {points, box, cell_start, (const KnnRow *)sorted, slabs, queries, valid, values, indices, dist2, mean,
                       N, nx, ny, nz, Q, k};
    hipStream_t s = (hipStream_t)stream;
    if (k == 1) knn_launch<1>(A, s);
    else if (k <= 4) knn_launch<4>(A, s);
    else if (k == 5) knn_launch<5>(A, s);
    else if (k <= 8) knn_launch<8>(A, s);
    else if (k == 9) knn_launch<9>(A, s);
    else knn_launch<16>(A, s);
    return lnh_check_launch("lnh_knn_search");
}

}  // extern "C"
