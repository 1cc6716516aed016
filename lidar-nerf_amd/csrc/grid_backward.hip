// grid_backward.hip — the grid encoder's atomic table backward (any D / C; training runs the bucketed backward of
// grid_bwd_scatter.hip / grid_bwd_reduce.hip instead), its input backward and the total-variation gradient.
//
// Atomic backward: packed `global_atomic_pk_add_f16` (fp16 tables) / `global_atomic_add_f32`, preceded by a wave-level
// run-merge: lanes whose sample falls in the same cell as their lower neighbour (the common case on coarse levels, where
// one cell spans many consecutive samples of a ray) are summed with a segmented shuffle scan and only the run tail
// issues the atomic.
#include "grid_pool.h"  // atomic_add_pair

namespace {

__device__ __forceinline__ void atomic_add_one(float *p, float a) { unsafeAtomicAdd(p, a); }

// One thread = one (point, level, channel pair).  NC = channels per thread (1 or 2).
// MERGE: wave-level run merge of equal cells before the atomics (see file header).
template <typename T, int D, int C, int NC, bool MERGE>
__global__ void __launch_bounds__(256)
k_grid_backward(const T *__restrict__ grad, const float *__restrict__ inputs, T *__restrict__ grad_table, uint32_t B,
                GridMeta meta, uint32_t align, uint32_t interp) {
    constexpr int NP = C / NC;  // channel groups per point
    const uint32_t level = blockIdx.y;
    const LevelParams lv = meta.lv[level];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = t / NP;
    const uint32_t ch = (t % NP) * NC;
    const bool in_range = b < B;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = in_range ? inputs[(size_t)b * D + d] : -1.0f;
    Cell<D> cell;
    const bool ok = in_range && locate<D>(x, lv, align != 0, interp, cell);
    float g[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) g[c] = ok ? (float)grad[((size_t)level * B + b) * C + ch + c] : 0.0f;
    T *gt = grad_table + (size_t)lv.offset * C + ch;

    if (MERGE && NP == 1) {
        // Lanes are consecutive samples.  If this lane's base cell equals the previous lane's, both touch the same
        // 2^D table rows: pre-reduce w*g over such runs with a segmented inclusive scan; the LAST lane of each run
        // issues the atomics.  Cell identity = all per-dimension base terms equal (exact, hash or dense).
        const int lane = threadIdx.x & 63;
        uint32_t key[D];
#pragma unroll
        for (int d = 0; d < D; d++) key[d] = ok ? cell.term[d][0] : 0xffffffffu - lane;  // invalid lanes never match
        // NB: every shuffle must execute with all 64 lanes active — no short-circuit around it
        bool same_prev = true;
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t up = __shfl_up(key[d], 1, 64);
            same_prev &= (up == key[d]);
        }
        same_prev &= lane > 0;
        const unsigned long long heads = __ballot(!same_prev);  // bit set where a run starts
        // distance to the start of my run
        const unsigned long long below = heads & ((2ull << lane) - 1ull);
        const int run_start = 63 - __builtin_clzll(below);
        const bool any_merge = (~heads) != 0ull;
        const unsigned long long heads_above = (lane == 63) ? 0ull : (heads >> (lane + 1));
        const bool is_tail = (lane == 63) || (heads_above & 1ull);
        if (any_merge) {  // wave-uniform
#pragma unroll
            for (uint32_t c = 0; c < (1u << D); c++) {
                const float w = ok ? corner_weight<D>(cell, c) : 0.0f;
                float v[NC];
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    v[k] = w * g[k];
                    if constexpr (sizeof(T) == 2) v[k] = (float)(half_t)v[k];  // per-contribution rounding (cu:350)
                }
#pragma unroll
                for (int k = 0; k < NC; k++) v[k] = wave_segscan_add(v[k], lane, run_start);
                if (ok && is_tail) {
                    T *p = gt + (size_t)corner_row<D>(cell, lv, c) * C;
                    if constexpr (NC == 2) atomic_add_pair(p, v[0], v[1]);
                    else atomic_add_one(p, v[0]);
                }
            }
            return;
        }
    }
    if (!ok) return;
#pragma unroll
    for (uint32_t c = 0; c < (1u << D); c++) {
        const float w = corner_weight<D>(cell, c);
        T *p = gt + (size_t)corner_row<D>(cell, lv, c) * C;
        if constexpr (NC == 2) atomic_add_pair(p, w * g[0], w * g[1]);
        else atomic_add_one(p, w * g[0]);
    }
}

// gridencoder.cu:364-390
template <typename T, int D, int C>
__global__ void k_grid_input_backward(const T *__restrict__ grad, const T *__restrict__ dy_dx,
                                      T *__restrict__ grad_inputs, uint32_t B, uint32_t L) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    T r = (T)0.0f;
    for (uint32_t l = 0; l < L; l++)
#pragma unroll
        for (int ch = 0; ch < C; ch++)
            r = (T)((float)r + (float)grad[((size_t)l * B + b) * C + ch] *
                                   (float)dy_dx[(((size_t)b * L + l) * D + d) * C + ch]);
    grad_inputs[t] = r;
}

// ------------------------------------------------------------------------------------------------ TV gradient
// gridencoder.cu:695-807
template <typename T, int D, int C>
__global__ void __launch_bounds__(256)
k_grad_tv(const T *__restrict__ inputs, const T *__restrict__ table, T *__restrict__ grad, float weight, uint32_t B,
          GridMeta meta, uint32_t align) {
    const uint32_t level = blockIdx.y;
    const LevelParams lv = meta.lv[level];
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float x[D];
#pragma unroll
    for (int d = 0; d < D; d++) x[d] = (float)inputs[(size_t)b * D + d];
    Cell<D> cell;
    if (!locate<D>(x, lv, align != 0, 0, cell)) return;
    const T *tab = table + (size_t)lv.offset * C;
    T *gt = grad + (size_t)lv.offset * C;
    // integer lattice position of the base corner and a row-index helper working on explicit coordinates
    uint32_t pg[D];
#pragma unroll
    for (int d = 0; d < D; d++) pg[d] = (uint32_t)floorf(fmaf(x[d], lv.scale, align ? 0.0f : 0.5f));
    auto row_of = [&](const uint32_t(&p)[D]) {
        const uint32_t R = (align || (lv.flags & LV_RSTRIDE)) ? lv.resolution : lv.resolution + 1;
        const uint32_t nd = lv.flags & 15u;
        uint32_t idx = 0, stride = 1;
        if (lv.flags & LV_HASH) {
#pragma unroll
            for (int d = 0; d < D; d++) idx ^= p[d] * prime_of(d);
        } else {
#pragma unroll
            for (int d = 0; d < D; d++)
                if ((uint32_t)d < nd) {
                    idx += p[d] * stride;
                    stride *= R;
                }
        }
        return idx % lv.hashmap_size;
    };
    const uint32_t index = row_of(pg) * C;
    float results[C], idelta[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) results[ch] = idelta[ch] = 0.0f;
    const T w = (T)(weight / (2 * D));
#pragma unroll
    for (int d = 0; d < D; d++) {
        const uint32_t cur = pg[d];
        if (cur < lv.resolution) {
            pg[d] = cur + 1;
            const uint32_t ir = row_of(pg) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                T gv = (T)(tab[index + ch] - tab[ir + ch]);
                results[ch] = (float)(T)(results[ch] + (float)gv);
                idelta[ch] = (float)(T)(idelta[ch] + (float)(T)(gv * gv));
            }
        }
        if (cur > 0) {
            pg[d] = cur - 1;
            const uint32_t il = row_of(pg) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) {
                T gv = (T)(tab[index + ch] - tab[il + ch]);
                results[ch] = (float)(T)(results[ch] + (float)gv);
                idelta[ch] = (float)(T)(idelta[ch] + (float)(T)(gv * gv));
            }
        }
        pg[d] = cur;
    }
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
        // `w * results[ch]` is a scalar_t product in the reference (rounded to the table type), then a float product
        const float v = (float)(T)((float)w * results[ch]) * rsqrtf(idelta[ch] + 1e-9f);
        if constexpr (sizeof(T) == 4) {
            unsafeAtomicAdd((float *)gt + index + ch, v);
        } else {
            // scalar fp16 atomic through the aligned packed instruction: add (v,0) or (0,v)
            half_t *p = (half_t *)gt + index + ch;
            const bool hi = ((uintptr_t)p & 2) != 0;
            half_t *pa = hi ? p - 1 : p;
            atomic_add_pair(pa, hi ? 0.0f : v, hi ? v : 0.0f);
        }
    }
}

template <typename T, int D>
int launch_backward_c(const T *grad, const float *inputs, T *ge, uint32_t B, uint32_t C, uint32_t L,
                      const GridMeta &m, uint32_t align, uint32_t interp, hipStream_t s) {
    const int rc = with_channels(C, [&](auto c) {
        // a thread owns NC channels of a point (a packed pair where there is one); the run-merge serves C <= 2
        constexpr int CC = decltype(c)::value, NC = CC == 1 ? 1 : 2;
        if constexpr (CC == 1 && sizeof(T) == 2) {
            lnh_set_error("grid backward: fp16 tables need an even C (the reference forces fp32 when C is odd, "
                          "grid.py:54-57)");
            return LNH_ERR_UNSUPPORTED;
        } else {
            LNH_LAUNCH((k_grid_backward<T, D, CC, NC, (CC <= 2)>), dim3(div_up((uint64_t)B * (CC / NC), 256), L), dim3(256), 0,
                       s, grad, inputs, ge, B, m, align, interp);
            return LNH_OK;
        }
    });
    return rc ? rc : lnh_check_launch("lnh_grid_encode_backward");
}

template <typename T, int D>
int launch_input_backward_c(const T *grad, const T *dy_dx, T *gi, uint32_t B, uint32_t C, uint32_t L, hipStream_t s) {
    const int rc = with_channels(C, [&](auto c) {
        LNH_LAUNCH((k_grid_input_backward<T, D, decltype(c)::value>), dim3(div_up((uint64_t)B * D, 256)), dim3(256), 0, s, grad,
                   dy_dx, gi, B, L);
        return LNH_OK;
    });
    return rc ? rc : lnh_check_launch("lnh_grid_encode_backward(inputs)");
}

template <typename T, int D>
int launch_tv_c(const T *inputs, const T *emb, T *grad, float weight, uint32_t B, uint32_t C, uint32_t L,
                const GridMeta &m, uint32_t align, hipStream_t s) {
    const int rc = with_channels(C, [&](auto c) {
        constexpr int CC = decltype(c)::value;
        if constexpr (CC == 1 && sizeof(T) == 2) {
            lnh_set_error("grad_total_variation: fp16 needs an even C");
            return LNH_ERR_UNSUPPORTED;
        } else {
            LNH_LAUNCH((k_grad_tv<T, D, CC>), dim3(div_up(B, 256), L), dim3(256), 0, s, inputs, emb, grad, weight, B, m, align);
            return LNH_OK;
        }
    });
    return rc ? rc : lnh_check_launch("lnh_grad_total_variation");
}

}  // namespace

extern "C" {

int lnh_grid_encode_backward(const void *grad, const float *inputs, const void *embeddings,
                             const int32_t *offsets_host, void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                             uint32_t L, float S, uint32_t H, const void *dy_dx, void *grad_inputs, uint32_t gridtype,
                             int align_corners, uint32_t interp, int dtype, lnh_stream_t stream) {
    (void)embeddings;
    int rc = check_common(inputs, offsets_host, B, D, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(grad && grad_embeddings, LNH_ERR_INVALID_ARG, "grid backward: null grad/grad_embeddings");
    LNH_REQUIRE((dy_dx == nullptr) == (grad_inputs == nullptr), LNH_ERR_INVALID_ARG,
                "grid backward: dy_dx and grad_inputs must be given together");
    if (B == 0) return LNH_OK;
    GridMeta m;
    if ((rc = resolve_levels(m, offsets_host, D, L, S, H, gridtype, align_corners))) return rc;
    hipStream_t s = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const int rc = with_dim(D, [&](auto d) {
            return launch_backward_c<T, decltype(d)::value>((const T *)grad, inputs, (T *)grad_embeddings, B, C, L, m,
                                                            align_corners != 0, interp, s);
        });
        if (rc != LNH_OK || !dy_dx) return rc;
        return with_dim(D, [&](auto d) {
            return launch_input_backward_c<T, decltype(d)::value>((const T *)grad, (const T *)dy_dx, (T *)grad_inputs, B, C, L, s);
        });
    });
}

int lnh_grad_total_variation(const void *inputs, const void *embeddings, void *grad, const int32_t *offsets_host,
                             float weight, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             uint32_t gridtype, int align_corners, int dtype, lnh_stream_t stream) {
    int rc = check_common(inputs, offsets_host, B, D, C, L, dtype);
    if (rc) return rc;
    LNH_REQUIRE(embeddings && grad, LNH_ERR_INVALID_ARG, "grad_total_variation: null embeddings/grad");
    if (B == 0) return LNH_OK;
    GridMeta m;
    if ((rc = resolve_levels(m, offsets_host, D, L, S, H, gridtype, align_corners))) return rc;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_dim(D, [&](auto d) {
            return launch_tv_c<T, decltype(d)::value>((const T *)inputs, (const T *)embeddings, (T *)grad, weight, B, C, L, m,
                                                      align_corners != 0, (hipStream_t)stream);
        });
    });
}

}  // extern "C"
