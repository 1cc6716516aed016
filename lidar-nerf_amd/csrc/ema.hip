// ema.hip — the exponential moving average of the parameters that the reference trains every run with (nerf/utils.py:
// 619-624 torch_ema.ExponentialMovingAverage(model.parameters(), 0.95); update() once per epoch, 1257-1258; the averaged
// weights swapped in for every evaluation and back out, 1297-1299 / 1444-1445) as two streaming kernels next to the
// optimizer pass of optim.hip: the 13.7 M-parameter table in the first blocks, the handful of small fp32 tensors (the MLP
// weights) in the blocks behind them, ONE launch for all parameters.
//   k_ema_update   s -= (s - p) * (1 - decay), three separately rounded fp32 operations in torch_ema's order
//                  (tmp = s - p; tmp *= 1 - decay; s -= tmp) — the library is built with -ffp-contract=off and no fmaf is
//                  written here, so the result is the torch formulation's to the last bit.  12 B per parameter.
//   k_ema_swap     p <-> s in place, and for the table the fp16 compute copy of the NEW p in the same pass: what
//                  store() + copy_to() before an evaluation and restore() after it do with a third copy of the parameters,
//                  without that copy, and with the fp16 table the render kernels read correct when the kernel finishes.
//                  Applied twice it is the identity.
#include "common.h"

namespace {

struct EmaSmall {
    float *a[LNH_TRAIN_MAX_SMALL], *b[LNH_TRAIN_MAX_SMALL];  // update: a = shadow, b = parameter; swap: the two sides
    uint32_t n[LNH_TRAIN_MAX_SMALL];
    uint32_t count;
};

struct EmaArgs {
    float *a, *b;  // table: update a = shadow (written), b = parameter (read); swap: a = parameter, b = shadow
    half_t *a16;   // swap only: fp16 copy of the new a (may be null)
    uint64_t n;
    EmaSmall s;
    float w;  // update only: 1 - decay
    uint32_t table_blocks;
};

__device__ __forceinline__ float ema_of(float s, float p, float w) {
    float tmp = s - p;
    tmp = tmp * w;
    return s - tmp;
}

__global__ void __launch_bounds__(256)
k_ema_update(EmaArgs a) {
    const float w = a.w;
    if (blockIdx.x < a.table_blocks) {
        const uint64_t n4 = a.n / 4;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)a.table_blocks * blockDim.x) {
            float4 s = reinterpret_cast<float4 *>(a.a)[i];
            const float4 p = reinterpret_cast<const float4 *>(a.b)[i];
            s.x = ema_of(s.x, p.x, w);
            s.y = ema_of(s.y, p.y, w);
            s.z = ema_of(s.z, p.z, w);
            s.w = ema_of(s.w, p.w, w);
            reinterpret_cast<float4 *>(a.a)[i] = s;
        }
        if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {  // tail
            const uint64_t i = n4 * 4 + threadIdx.x;
            a.a[i] = ema_of(a.a[i], a.b[i], w);
        }
        return;
    }
    // small tensors: the blocks behind the table's walk all of them together
    const uint32_t nb = gridDim.x - a.table_blocks, b = blockIdx.x - a.table_blocks;
    for (uint32_t k = 0; k < a.s.count; k++)
        for (uint32_t i = b * blockDim.x + threadIdx.x; i < a.s.n[k]; i += nb * blockDim.x)
            a.s.a[k][i] = ema_of(a.s.a[k][i], a.s.b[k][i], w);
}

__global__ void __launch_bounds__(256)
k_ema_swap(EmaArgs a) {
    if (blockIdx.x < a.table_blocks) {
        const uint64_t n4 = a.n / 4;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)a.table_blocks * blockDim.x) {
            const float4 p = reinterpret_cast<const float4 *>(a.a)[i], s = reinterpret_cast<const float4 *>(a.b)[i];
            reinterpret_cast<float4 *>(a.a)[i] = s;
            reinterpret_cast<float4 *>(a.b)[i] = p;
            if (a.a16) {
                half4_t h;
                h[0] = (half_t)s.x; h[1] = (half_t)s.y; h[2] = (half_t)s.z; h[3] = (half_t)s.w;
                reinterpret_cast<half4_t *>(a.a16)[i] = h;
            }
        }
        if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {  // tail
            const uint64_t i = n4 * 4 + threadIdx.x;
            const float p = a.a[i], s = a.b[i];
            a.a[i] = s;
            a.b[i] = p;
            if (a.a16) a.a16[i] = (half_t)s;
        }
        return;
    }
    const uint32_t nb = gridDim.x - a.table_blocks, b = blockIdx.x - a.table_blocks;
    for (uint32_t k = 0; k < a.s.count; k++)
        for (uint32_t i = b * blockDim.x + threadIdx.x; i < a.s.n[k]; i += nb * blockDim.x) {
            const float p = a.s.a[k][i], s = a.s.b[k][i];
            a.s.a[k][i] = s;
            a.s.b[k][i] = p;
        }
}

// argument checks and grid of both entry points (table blocks first, capped like k_train_step; at most 64 blocks behind
// them for the small tensors); returns 0 blocks when there is nothing to do
int ema_args(EmaArgs &a, uint32_t &blocks, float *ta, float *tb, void *a16, uint64_t n, float *const *sa, float *const *sb,
             const uint32_t *numel, uint32_t n_small, const char *who) {
    LNH_REQUIRE(n == 0 || (ta && tb), LNH_ERR_INVALID_ARG, "%s: null table pointer", who);
    LNH_REQUIRE(n == 0 || ta != tb, LNH_ERR_INVALID_ARG, "%s: parameter and shadow must be different buffers", who);
    LNH_REQUIRE(n == 0 || ((((uintptr_t)ta | (uintptr_t)tb) & 15) == 0 && ((uintptr_t)a16 & 7) == 0), LNH_ERR_INVALID_ARG,
                "%s: buffers must be 16-byte (fp32) / 8-byte (fp16) aligned", who);
    LNH_REQUIRE(n_small <= LNH_TRAIN_MAX_SMALL && (n_small == 0 || (sa && sb && numel)), LNH_ERR_INVALID_ARG,
                "%s: at most %d small tensors", who, LNH_TRAIN_MAX_SMALL);
    a.a = ta; a.b = tb; a.a16 = (half_t *)a16; a.n = n;
    a.s.count = n_small;
    uint32_t small_max = 0;
    for (uint32_t k = 0; k < n_small; k++) {
        LNH_REQUIRE(numel[k] == 0 || (sa[k] && sb[k]), LNH_ERR_INVALID_ARG, "%s: null small-tensor pointer %u", who, k);
        LNH_REQUIRE((((uintptr_t)sa[k] | (uintptr_t)sb[k]) & 3) == 0, LNH_ERR_INVALID_ARG,
                    "%s: small tensor %u must be 4-byte aligned", who, k);
        LNH_REQUIRE(numel[k] == 0 || sa[k] != sb[k], LNH_ERR_INVALID_ARG, "%s: small tensor %u: parameter and shadow must be "
                    "different buffers", who, k);
        a.s.a[k] = sa[k]; a.s.b[k] = sb[k]; a.s.n[k] = numel[k];
        small_max = small_max > numel[k] ? small_max : numel[k];
    }
    const uint64_t n4 = n / 4;
    a.table_blocks = n ? (uint32_t)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 + 1 : 4096) : 0;
    const uint32_t small_blocks = (small_max + 255) / 256;
    blocks = a.table_blocks + (small_blocks > 64 ? 64 : small_blocks);
    return LNH_OK;
}
}  // namespace

extern "C" {

int lnh_ema_update(float *shadow, const float *param, uint64_t n, float *const *small_shadow, const float *const *small_param,
                   const uint32_t *small_numel, uint32_t n_small, float one_minus_decay, lnh_stream_t stream) {
    EmaArgs a{};
    uint32_t blocks = 0;
    if (int rc = ema_args(a, blocks, shadow, const_cast<float *>(param), nullptr, n, small_shadow,
                          const_cast<float *const *>(small_param), small_numel, n_small, "ema_update"))
        return rc;
    LNH_REQUIRE(one_minus_decay >= 0.0f && one_minus_decay <= 1.0f, LNH_ERR_INVALID_ARG,
                "ema_update: one_minus_decay must lie in [0, 1]");
    if (blocks == 0) return LNH_OK;
    a.w = one_minus_decay;
    LNH_LAUNCH(k_ema_update, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_ema_update");
}

int lnh_ema_swap(float *param, float *shadow, void *param16, uint64_t n, float *const *small_param, float *const *small_shadow,
                 const uint32_t *small_numel, uint32_t n_small, lnh_stream_t stream) {
    EmaArgs a{};
    uint32_t blocks = 0;
    if (int rc = ema_args(a, blocks, param, shadow, param16, n, small_param, small_shadow, small_numel, n_small, "ema_swap"))
        return rc;
    if (blocks == 0) return LNH_OK;
    LNH_LAUNCH(k_ema_swap, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_ema_swap");
}

}  // extern "C"
