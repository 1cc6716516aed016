// cell_grid.h — the uniform grid of cells over a bounding box that raycast.hip and knn.hip build and walk, once.
// Their exactness arguments rest on the build and the search sharing ONE monotone cell_of: this is it.
//   plain C++ part   cell_finite, CellGrid, cell_grid, cell_of: also compiles without hipcc (knn_walk.h includes it,
//                    tools/knn_walk_host.cpp runs it on the host)
//   device part      the bounds passes: per-thread min / max / bad-coordinate count over an [N,3] array, the 256-thread reduce
//                    into a partial of words, the merge of the partials by one workgroup
//   host part        the checks of a grid and of a workspace, with the error strings both features report
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include "common.h"
#define LNH_HD __host__ __device__ __forceinline__
#else
#define LNH_HD inline
#endif

LNH_HD bool cell_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

struct CellGrid {
    float lo[3], inv[3];
    uint32_t n[3];
};
// The grid of nx x ny x nz cells over the box (lo[3], hi[3]).  e = max(hi[a] - lo[a], largest extent * 2^-10) is the floored
// extent of axis a (1 when the box is a single point), inv[a] = n[a] / e.  on_extent(a, e) is called with that e just before
// inv[a] is formed: a caller that derives more from the same e (raycast.hip: the cell width e / n[a]) does it there.
template <typename OnExtent>
LNH_HD CellGrid cell_grid(const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz, OnExtent on_extent) {
    CellGrid g;
    g.n[0] = nx, g.n[1] = ny, g.n[2] = nz;
    float emax = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g.lo[a] = box[a];
        emax = fmaxf(emax, box[3 + a] - box[a]);
    }
    if (!(emax > 0.0f) || !cell_finite(emax)) emax = 1.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float e = fmaxf(box[3 + a] - box[a], emax * 0.0009765625f);
        on_extent(a, e);
        g.inv[a] = (float)g.n[a] / e;
    }
    return g;
}
LNH_HD CellGrid cell_grid(const float *__restrict__ box, uint32_t nx, uint32_t ny, uint32_t nz) {
    return cell_grid(box, nx, ny, nz, [](int, float) {});
}
LNH_HD uint32_t cell_of(float x, float lo, float inv, uint32_t n) {
    const float c = floorf((x - lo) * inv);
    return (uint32_t)fminf(fmaxf(c, 0.0f), (float)(n - 1));  // (a NaN becomes cell 0)
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------- device part
constexpr uint32_t kCellThreads = 256;  // workgroup of the bounds passes
constexpr uint32_t kCellBoundsGroupsMax = 1024;
constexpr uint32_t kCellMaxPerAxis = 1024;

// The bounds of an array come out of two launches without atomics: every workgroup writes a partial, one workgroup folds them.
// A partial is NF floats (the first three are minima, the others maxima), NU counters and one zero word: NF + NU + 1 words.

// this thread's share of an [N,3] array, grid stride: lo[3] / hi[3] of the finite coordinates, the others counted in `bad`
__device__ __forceinline__ void cell_bounds_accumulate(const float *__restrict__ xyz, uint32_t N, float *lo, float *hi,
                                                       uint32_t &bad) {
    const uint32_t stride = gridDim.x * kCellThreads;
    for (uint32_t i = blockIdx.x * kCellThreads + threadIdx.x; i < N; i += stride) {  // (i + stride < 2^32: N < 2^31, stride <= 2^18)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float x = xyz[(size_t)i * 3 + a];
            if (cell_finite(x))
                lo[a] = fminf(lo[a], x), hi[a] = fmaxf(hi[a], x);
            else
                bad++;
        }
    }
}
// min / max / sums over the 256 threads; thread 0 writes the words of the partial
template <int NF, int NU>
__device__ __forceinline__ void cell_block_reduce(float (&f)[NF], uint32_t (&u)[NU], uint32_t *__restrict__ out) {
    __shared__ float s_f[4][NF];
    __shared__ uint32_t s_u[4][NU];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NF; a++) f[a] = a < 3 ? wave_min(f[a]) : wave_max(f[a]);
#pragma unroll
    for (int c = 0; c < NU; c++) u[c] = wave_sum(u[c]);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < NF; a++) s_f[wv][a] = f[a];
#pragma unroll
        for (int c = 0; c < NU; c++) s_u[wv][c] = u[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < NF; a++) {
            float v = s_f[0][a];
            for (int w = 1; w < 4; w++) v = a < 3 ? fminf(v, s_f[w][a]) : fmaxf(v, s_f[w][a]);
            out[a] = __float_as_uint(v);
        }
#pragma unroll
        for (int c = 0; c < NU; c++) out[NF + c] = s_u[0][c] + s_u[1][c] + s_u[2][c] + s_u[3][c];
        out[NF + NU] = 0u;
    }
}
// this thread's share of the G partials of the workgroups, folded into f and u (preset by the caller), ready for the reduce
template <int NF, int NU>
__device__ __forceinline__ void cell_merge_partials(const uint32_t *__restrict__ partials, uint32_t G, float (&f)[NF],
                                                    uint32_t (&u)[NU]) {
    for (uint32_t g = threadIdx.x; g < G; g += kCellThreads) {
        const uint32_t *p = partials + (size_t)g * (NF + NU + 1);
#pragma unroll
        for (int a = 0; a < NF; a++) f[a] = a < 3 ? fminf(f[a], __uint_as_float(p[a])) : fmaxf(f[a], __uint_as_float(p[a]));
        // a count that does not fit 32 bits saturates
#pragma unroll
        for (int c = 0; c < NU; c++) u[c] = u[c] + p[NF + c] < u[c] ? 0xffffffffu : u[c] + p[NF + c];
    }
#pragma unroll
    for (int c = 0; c < NU; c++) u[c] = min(u[c], 0xffffffu);  // (256 * 2^24 fits; nonzero stays nonzero)
}

// ------------------------------------------------------------------------------------------------------------ host part
static inline bool cell_grid_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= kCellMaxPerAxis && ny <= kCellMaxPerAxis && nz <= kCellMaxPerAxis;
}
// workgroups of a bounds pass over n items
static inline uint32_t cell_bounds_groups(uint32_t n) {
    const uint32_t g = div_up(n, kCellThreads);
    return g < 1 ? 1 : (g > kCellBoundsGroupsMax ? kCellBoundsGroupsMax : g);
}
static inline int cell_check_grid(const char *who, const float *box, uint32_t nx, uint32_t ny, uint32_t nz) {
    LNH_REQUIRE(box && ((uintptr_t)box & 3) == 0, LNH_ERR_INVALID_ARG, "%s: null pointer (box)", who);
    LNH_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, LNH_ERR_INVALID_ARG, "%s: grid of %u x %u x %u cells, every dimension must be >= 1",
                who, nx, ny, nz);
    LNH_REQUIRE(cell_grid_ok(nx, ny, nz), LNH_ERR_UNSUPPORTED, "%s: grid of %u x %u x %u cells, at most %u per axis", who, nx, ny, nz,
                kCellMaxPerAxis);
    return LNH_OK;
}
static inline int cell_check_ws(const char *who, uint64_t need, const void *ws, uint64_t ws_bytes) {
    LNH_REQUIRE(ws && ((uintptr_t)ws & 3) == 0 && ws_bytes >= need, LNH_ERR_INVALID_ARG,
                "%s: workspace of %llu bytes (4-byte aligned) needed, got %llu", who, (unsigned long long)need,
                (unsigned long long)ws_bytes);
    return LNH_OK;
}
#endif  // __HIPCC__
