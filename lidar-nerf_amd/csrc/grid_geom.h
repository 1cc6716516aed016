// grid_geom.h — level geometry of the multi-resolution hash / tiled grid encoder, shared by every grid_*.hip.
//
// Semantics follow the reference kernels (lidarnerf/gridencoder/src/gridencoder.cu:53-390, 695-807).  The level geometry
// (scale, resolution, dense/hash decision, modulo strategy) is resolved ONCE on the host (build_meta) and handed to the
// kernels in kernarg SGPRs, so the per-corner index math (locate, corner_row) is a handful of VALU ops with no per-thread
// loop-carried stride test and no integer division on the hot levels.  Also here: the small vector load / store helpers,
// the host dispatch on the kernels' template arguments, and the front checks every entry point starts with.
//   grid_forward.hip      the encode forward and its schedule
//   grid_backward.hip     the atomic backward (any D / C; training does not use it), the input backward, the TV gradient
//   grid_bwd_scatter.hip  pass 1 of the bucketed backward (what training runs)  \  their contract: grid_pool.h
//   grid_bwd_reduce.hip   pass 2, the workspace plan, the entry points          /
#pragma once
#include "common.h"

#include <type_traits>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

// (LevelParams, GridMeta and BucketPlan — grid_pool.h — cross a translation-unit boundary as arguments of the scatter
//  launcher, so they have linkage; everything else of the grid files lives in anonymous namespaces)
struct LevelParams {
    float scale;
    uint32_t resolution;
    uint32_t hashmap_size;
    uint32_t offset;  // rows before this level
    uint32_t flags;   // bits 0-3: dims accumulated densely; bit4 hash; bit5 pow2 table; bit6 no wrap needed;
                      // bit7 lattice stride = resolution (tiny-cuda-nn); bit8 wrap by one compare-and-subtract
};
struct GridMeta {
    LevelParams lv[LNH_MAX_LEVELS];
};

namespace {

enum { LV_HASH = 16, LV_POW2 = 32, LV_NOWRAP = 64, LV_RSTRIDE = 128, LV_WRAP1 = 256 };
// gridtype 2: tiny-cuda-nn's lattice (its published GridEncoding: grid_index / pos_fract, restated; parity with a real
// tiny-cuda-nn build is unpinned).  Same scale, resolution, hash and cell position as gridtype 0, but a dense level has
// stride `resolution` (not resolution + 1) and its rows ALWAYS wrap modulo the level's rows: the +1 corner of the last cell
// (x = resolution) aliases the next row, exactly as tiny-cuda-nn does.  A dense level there has idx <= res + ... + res^D <
// 2 * rows, so the modulo is one compare-and-subtract (LV_WRAP1); a hashed level has rows = 2^log2_hashmap_size (mask).
enum { kGridHash = 0, kGridTiled = 1, kGridTcnn = 2 };

// gridencoder.cu:55-57 (spatial-hash primes); folded to immediates after unrolling
__host__ __device__ constexpr uint32_t prime_of(int d) {
    return d == 0 ? 1u : d == 1 ? 2654435761u : d == 2 ? 805459861u : d == 3 ? 3674653429u
         : d == 4 ? 2097192037u : d == 5 ? 1434869437u : 2165219737u;
}

// Host: gridencoder.cu:146-148 + the stride loop of get_grid_index (69-84) evaluated once per level.
// exp2f(level*S) is evaluated in double and rounded once (same convention as the oracle).
int build_meta(GridMeta &m, const int32_t *offsets, uint32_t D, uint32_t L, float S, uint32_t H, uint32_t gridtype,
               bool align) {
    if (gridtype > kGridTcnn || (gridtype == kGridTcnn && align)) return -1;  // tiny-cuda-nn has no align_corners
    const bool tcnn = gridtype == kGridTcnn;
    for (uint32_t l = 0; l < L; l++) {
        LevelParams &p = m.lv[l];
        float e = (float)l * S;
        float pw = (float)exp2((double)e);
        p.scale = pw * (float)H - 1.0f;
        p.resolution = (uint32_t)ceilf(p.scale) + 1u;
        int64_t hm = (int64_t)offsets[l + 1] - (int64_t)offsets[l];
        if (hm <= 0 || offsets[l] < 0) return -1;
        p.hashmap_size = (uint32_t)hm;
        p.offset = (uint32_t)offsets[l];
        uint32_t R = (align || tcnn) ? p.resolution : p.resolution + 1;
        uint32_t stride = 1, nd = 0;
        uint64_t exact = 1;
        for (uint32_t d = 0; d < D && stride <= p.hashmap_size; d++) {
            stride *= R;  // uint32 wrap-around exactly like the device code it replaces
            exact *= R;
            nd++;
        }
        uint32_t f = nd;
        bool hash = (gridtype != kGridTiled && stride > p.hashmap_size);
        if (hash) f |= LV_HASH;
        if ((p.hashmap_size & (p.hashmap_size - 1)) == 0) f |= LV_POW2;
        if (tcnn) {
            f |= LV_RSTRIDE;
            // largest index of a dense level: every coordinate at R (the +1 corner of the last cell) -> R + R^2 + .. + R^D
            uint64_t top = 0, pw = 1;
            for (uint32_t d = 0; d < nd; d++) top += (pw *= R);
            if (!hash && top < 2ull * p.hashmap_size) f |= LV_WRAP1;
        } else if (!hash && nd == D && exact <= p.hashmap_size) {
            f |= LV_NOWRAP;
        }
        p.flags = f;
    }
    return 0;
}

template <int D>
struct Cell {
    uint32_t term[D][2];  // per-dimension contribution to the row index for offset 0 / +1
    float frac[D];
    float deriv[D];
};

// Position inside the level lattice (gridencoder.cu:150-167).  Returns false for out-of-range points.
template <int D>
__device__ __forceinline__ bool locate(const float (&x)[D], const LevelParams &lv, bool align, uint32_t interp,
                                       Cell<D> &c) {
    bool ok = true;
#pragma unroll
    for (int d = 0; d < D; d++) ok = ok && !(x[d] < 0.0f || x[d] > 1.0f);
    if (!ok) return false;
    const uint32_t R = (align || (lv.flags & LV_RSTRIDE)) ? lv.resolution : lv.resolution + 1;
    const bool hash = lv.flags & LV_HASH;
    const uint32_t nd = lv.flags & 15u;
    uint32_t stride = 1;
#pragma unroll
    for (int d = 0; d < D; d++) {
        float p = fmaf(x[d], lv.scale, align ? 0.0f : 0.5f);
        float fl = floorf(p);
        uint32_t g = (uint32_t)fl;
        p -= (float)g;
        if (interp == 1) {
            c.deriv[d] = 6.0f * p * (1.0f - p);
            p = p * p * (3.0f - 2.0f * p);
        } else {
            c.deriv[d] = 1.0f;
        }
        c.frac[d] = p;
        if (hash) {
            uint32_t t0 = g * prime_of(d);
            c.term[d][0] = t0;
            c.term[d][1] = t0 + prime_of(d);
        } else if ((uint32_t)d < nd) {
            uint32_t t0 = g * stride;
            c.term[d][0] = t0;
            c.term[d][1] = t0 + stride;
            stride *= R;
        } else {  // tiled grid whose stride already exceeded the table: dimension ignored (gridencoder.cu:81)
            c.term[d][0] = 0;
            c.term[d][1] = 0;
        }
    }
    return true;
}

template <int D>
__device__ __forceinline__ uint32_t corner_row(const Cell<D> &c, const LevelParams &lv, uint32_t corner) {
    uint32_t idx = 0;
    if (lv.flags & LV_HASH) {
#pragma unroll
        for (int d = 0; d < D; d++) idx ^= c.term[d][(corner >> d) & 1];
    } else {
#pragma unroll
        for (int d = 0; d < D; d++) idx += c.term[d][(corner >> d) & 1];
    }
    if (lv.flags & LV_POW2) idx &= lv.hashmap_size - 1;
    else if (lv.flags & LV_WRAP1) idx = idx >= lv.hashmap_size ? idx - lv.hashmap_size : idx;
    else if (!(lv.flags & LV_NOWRAP)) idx %= lv.hashmap_size;
    return idx;
}

template <int D>
__device__ __forceinline__ float corner_weight(const Cell<D> &c, uint32_t corner) {
    float w = 1.0f;
#pragma unroll
    for (int d = 0; d < D; d++) w *= ((corner >> d) & 1) ? c.frac[d] : (1.0f - c.frac[d]);
    return w;
}

template <typename T, int C>
struct Vec {
    T v[C];
};
template <typename T, int C>
__device__ __forceinline__ Vec<T, C> load_vec(const T *p) {
    Vec<T, C> r;
    if constexpr (sizeof(T) * C == 4) {
        uint32_t raw = *reinterpret_cast<const uint32_t *>(p);
        __builtin_memcpy(&r, &raw, 4);
    } else if constexpr (sizeof(T) * C == 8) {
        uint2 raw = *reinterpret_cast<const uint2 *>(p);
        __builtin_memcpy(&r, &raw, 8);
    } else if constexpr (sizeof(T) * C == 16) {
        uint4 raw = *reinterpret_cast<const uint4 *>(p);
        __builtin_memcpy(&r, &raw, 16);
    } else if constexpr (sizeof(T) * C == 32) {
        uint4 a = reinterpret_cast<const uint4 *>(p)[0], b = reinterpret_cast<const uint4 *>(p)[1];
        __builtin_memcpy(&r, &a, 16);
        __builtin_memcpy(reinterpret_cast<char *>(&r) + 16, &b, 16);
    } else {
#pragma unroll
        for (int i = 0; i < C; i++) r.v[i] = p[i];
    }
    return r;
}
template <typename T, int C>
__device__ __forceinline__ void store_vec(T *p, const Vec<T, C> &r) {
    if constexpr (sizeof(T) * C == 4) {
        uint32_t raw;
        __builtin_memcpy(&raw, &r, 4);
        *reinterpret_cast<uint32_t *>(p) = raw;
    } else if constexpr (sizeof(T) * C == 8) {
        uint2 raw;
        __builtin_memcpy(&raw, &r, 8);
        *reinterpret_cast<uint2 *>(p) = raw;
    } else if constexpr (sizeof(T) * C == 16) {
        uint4 raw;
        __builtin_memcpy(&raw, &r, 16);
        *reinterpret_cast<uint4 *>(p) = raw;
    } else {
#pragma unroll
        for (int i = 0; i < C; i++) p[i] = r.v[i];
    }
}

// Host dispatch on the runtime values the kernels take as template arguments: f receives the value as a
// std::integral_constant (the element type as a value of that type), and is instantiated for the listed cases only.
template <int N>
using Int = std::integral_constant<int, N>;
template <typename F>
int with_channels(uint32_t C, F f) {
    switch (C) {
        case 1: return f(Int<1>{});
        case 2: return f(Int<2>{});
        case 4: return f(Int<4>{});
        case 8: return f(Int<8>{});
    }
    lnh_set_error("GridEncoding: C must be 1, 2, 4, or 8 (got %u)", C);
    return LNH_ERR_UNSUPPORTED;
}
template <typename F>
int with_dim(uint32_t D, F f) {
    switch (D) {
        case 2: return f(Int<2>{});
        case 3: return f(Int<3>{});
        case 4: return f(Int<4>{});
        case 5: return f(Int<5>{});
    }
    return LNH_ERR_UNSUPPORTED;
}
template <typename F>
int with_dtype(int dtype, F f) {  // dtype has passed check_common
    return dtype == LNH_F32 ? f(float{}) : f(half_t{});
}

// The front of every entry point is check_common, the entry point's own argument checks, `B == 0` (nothing to do: LNH_OK
// whatever the geometry), then resolve_levels — in that order, which is the order callers see errors in.
int check_common(const void *inputs, const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                 int dtype) {
    LNH_REQUIRE(inputs && offsets_host, LNH_ERR_INVALID_ARG, "grid: null inputs/offsets");
    LNH_REQUIRE(L >= 1 && L <= LNH_MAX_LEVELS, LNH_ERR_UNSUPPORTED, "grid: L must be in 1..%d (got %u)", LNH_MAX_LEVELS, L);
    LNH_REQUIRE(D >= 2 && D <= 5, LNH_ERR_UNSUPPORTED, "GridEncoding: D must be 2, 3, 4 or 5 (got %u)", D);
    LNH_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8, LNH_ERR_UNSUPPORTED, "GridEncoding: C must be 1, 2, 4, or 8 (got %u)", C);
    LNH_REQUIRE(dtype == LNH_F32 || dtype == LNH_F16, LNH_ERR_UNSUPPORTED, "grid: dtype must be LNH_F32 or LNH_F16");
    (void)B;
    return LNH_OK;
}
int resolve_levels(GridMeta &m, const int32_t *offsets_host, uint32_t D, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                   int align_corners) {
    LNH_REQUIRE(build_meta(m, offsets_host, D, L, S, H, gridtype, align_corners != 0) == 0, LNH_ERR_INVALID_ARG,
                "grid: offsets must be increasing and non-negative, gridtype 0 / 1 / 2 (2: align_corners off)");
    return LNH_OK;
}

}  // namespace
