// unet_train_step.hip — what turns the ray-drop U-Net's forward and backward into a training step (DESIGN §19,
// raydrop_train_poisson.py:75-259): the loss and its cotangent in closed form, the sum of squares of all gradients, and
// clip_grad_norm_ + torch.optim.RMSprop(foreach=True) over a device-resident table of tensors in one launch.
//   lnh_unet_loss_grad     BCE-with-logits (mean) + 1 - dice(sigmoid(x), t) over the whole batch and dL/dx x loss_scale.  Two
//                          launches: float64 partials (BCE sum, I = sum s t, S = sum (s + t)) per workgroup, then every workgroup
//                          re-sums the partials in ascending order, forms the scalars and writes its slice.  Every element is formed
//                          in float64 (M is a frame's pixel count: the arithmetic costs nothing) and rounded to f32 once.
//   lnh_unet_grad_sumsq    sum g^2 over the table's gradients as one float64: kSumBlocks partials, finished in ascending order.
//   lnh_unet_rmsprop_step  unscale, clip, weight decay, square_avg, momentum_buffer, parameter — fp32 per element, each operation
//                          rounded on its own (the library is built with -ffp-contract=off) in the order torch applies them.
// No float atomics, no host read, no allocation; every sum's order depends on the sizes alone.  (unet_common.h: aligned16 and the
// 2^26 bound; the partial rule of the loss is this file's.)
#include <cmath>

#include "unet_common.h"

namespace {

constexpr uint32_t kT = 256;
constexpr uint32_t kLossMaxParts = 256;  // pass two re-sums them in every workgroup
constexpr uint32_t kChunk = 4096;        // elements of one tensor a workgroup takes at a time: 4 float4 per thread
constexpr uint32_t kSumBlocks = 1024;    // partials of grad_sumsq
constexpr uint32_t kStepBlocks = 2048;

// elements per workgroup of the loss kernels, from M alone: 256 up to 2^16 elements, then as many as keep the partials at 256
inline uint64_t loss_block_elems(uint64_t M) { return kT * ((M + (uint64_t)kT * kLossMaxParts - 1) / ((uint64_t)kT * kLossMaxParts)); }
inline uint32_t loss_parts(uint64_t M) { return (uint32_t)((M + loss_block_elems(M) - 1) / loss_block_elems(M)); }

template <bool kU8>
__device__ __forceinline__ double mask_at(const void *masks, uint64_t i) {
    if constexpr (kU8) return (double)reinterpret_cast<const uint8_t *>(masks)[i];
    else return (double)reinterpret_cast<const float *>(masks)[i];
}

template <bool kU8>
__global__ void __launch_bounds__(kT)
k_unet_loss_partials(const float *__restrict__ logits, const void *__restrict__ masks, uint64_t M, uint64_t E, double *__restrict__ ws) {
    __shared__ double sh[4];
    const uint64_t lo = (uint64_t)blockIdx.x * E, hi = lo + E < M ? lo + E : M;
    double bce = 0.0, I = 0.0, S = 0.0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kT) {
        const double x = (double)logits[i], t = mask_at<kU8>(masks, i);
        const double e = exp(-fabs(x));
        const double s = (x >= 0.0 ? 1.0 : e) / (1.0 + e);
        bce += fmax(x, 0.0) - x * t + log1p(e);
        I += s * t;
        S += s + t;
    }
    bce = block_sum<kT>(bce, sh);
    I = block_sum<kT>(I, sh);
    S = block_sum<kT>(S, sh);
    if (threadIdx.x == 0) {
        ws[3 * blockIdx.x] = bce;
        ws[3 * blockIdx.x + 1] = I;
        ws[3 * blockIdx.x + 2] = S;
    }
}

template <bool kU8>
__global__ void __launch_bounds__(kT)
k_unet_loss_grad(const float *__restrict__ logits, const void *__restrict__ masks, uint64_t M, uint64_t E, const double *__restrict__ ws,
                 double loss_scale, float *__restrict__ loss, float *__restrict__ dlogits) {
    double bce = 0.0, I = 0.0, S = 0.0;
    for (uint32_t k = 0; k < gridDim.x; k++) {  // ascending, the same chain in every workgroup
        bce += ws[3 * k];
        I += ws[3 * k + 1];
        S += ws[3 * k + 2];
    }
    const double eps = 1e-6, den = S + eps, num = 2.0 * I + eps, inv_m = 1.0 / (double)M;
    const bool empty = S == 0.0;  // dice_coeff's masked_fill: a pair of empty sets scores 1 and has no gradient
    if (blockIdx.x == 0 && threadIdx.x == 0) loss[0] = (float)(bce * inv_m + (1.0 - (empty ? 1.0 : num / den)));
    const double inv_den2 = 1.0 / (den * den);
    const uint64_t lo = (uint64_t)blockIdx.x * E, hi = lo + E < M ? lo + E : M;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += kT) {
        const double x = (double)logits[i], t = mask_at<kU8>(masks, i);
        const double e = exp(-fabs(x));
        const double s = (x >= 0.0 ? 1.0 : e) / (1.0 + e);
        const double ds = e / ((1.0 + e) * (1.0 + e));  // s (1 - s), from exp(-|x|): no digits lost where s is near 1
        const double dice = empty ? 0.0 : ds * (2.0 * t * den - num) * inv_den2;
        dlogits[i] = (float)(((s - t) * inv_m - dice) * loss_scale);
    }
}

// ---- the table of tensors -----------------------------------------------------------------------------------------------------------
// chunk prefix of the table in LDS: pre[k] = chunks of tensors 0 .. k - 1 (kChunk elements each, the last of a tensor ragged)
__device__ __forceinline__ uint32_t table_prefix(const lnh_urs_tensor *__restrict__ table, uint32_t n, uint32_t *pre) {
    if (threadIdx.x < 64) {
        const uint32_t k = threadIdx.x;
        uint32_t c = k < n ? (uint32_t)((table[k].numel + kChunk - 1) / kChunk) : 0u;
        c = wave_scan_add_u32(c);
        pre[k + 1] = c;
        if (k == 0) pre[0] = 0;
    }
    __syncthreads();
    return pre[64];
}
// the tensor chunk c belongs to: the last k with pre[k] <= c
__device__ __forceinline__ uint32_t table_find(const uint32_t *pre, uint32_t c) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t s = 32; s > 0; s >>= 1)
        if (k + s < 64 && pre[k + s] <= c) k += s;
    return k;
}

// Thread t of a chunk owns the float4 numbers t, t + 256, t + 512, t + 768 of it, whether they are read as float4 (the tensor
// starts on 16 bytes) or as scalars: the order of every sum is the same in both paths.
__global__ void __launch_bounds__(kT)
k_unet_grad_sumsq(const lnh_urs_tensor *__restrict__ table, uint32_t n, double *__restrict__ ws) {
    __shared__ uint32_t pre[65];
    __shared__ double sh[4];
    const uint32_t total = table_prefix(table, n, pre);
    double acc = 0.0;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
        const uint32_t k = table_find(pre, c);
        const uint64_t off = (uint64_t)(c - pre[k]) * kChunk, left = table[k].numel - off;
        const uint32_t m = left < kChunk ? (uint32_t)left : kChunk;
        const float *g = table[k].grad + off;
        if (aligned16(g)) {
            float4 v[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t q = threadIdx.x + kT * j;
                v[j] = 4 * q + 3 < m ? reinterpret_cast<const float4 *>(g)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t q = threadIdx.x + kT * j;
                if (4 * q + 3 < m) {
                    acc += (double)v[j].x * (double)v[j].x;
                    acc += (double)v[j].y * (double)v[j].y;
                    acc += (double)v[j].z * (double)v[j].z;
                    acc += (double)v[j].w * (double)v[j].w;
                } else {
                    for (uint32_t i = 4 * q; i < m; i++) acc += (double)g[i] * (double)g[i];  // the tail: at most 3, one thread
                }
            }
        } else {
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t q = threadIdx.x + kT * j;
                for (uint32_t i = 4 * q; i < 4 * q + 4 && i < m; i++) acc += (double)g[i] * (double)g[i];
            }
        }
    }
    acc = block_sum<kT>(acc, sh);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(kT)
k_unet_grad_sumsq_finish(const double *__restrict__ ws, double *__restrict__ state) {
    __shared__ double sh[kSumBlocks];
    for (uint32_t i = threadIdx.x; i < kSumBlocks; i += kT) sh[i] = ws[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (uint32_t i = 0; i < kSumBlocks; i++) s += sh[i];  // ascending
        state[LNH_URS_SUMSQ] = s;
        state[LNH_URS_NONFINITE] = (s - s == 0.0) ? 0.0 : 1.0;  // a square cannot cancel: the sum is finite iff every element is
    }
}

struct StepHyper {
    double loss_scale, max_norm;
    float inv_scale, alpha, one_minus_alpha, eps, wd, momentum;
};

__device__ __forceinline__ void rmsprop_elem(float &p, float g, float &sq, float &buf, const StepHyper &h, float coef, float neg_lr) {
    g = g * h.inv_scale;
    g = g * coef;
    if (h.wd != 0.0f) g = g + h.wd * p;
    sq = sq * h.alpha;
    sq = sq + (h.one_minus_alpha * g) * g;
    const float avg = sqrtf(sq) + h.eps;
    if (h.momentum > 0.0f) {
        buf = buf * h.momentum;
        buf = buf + g / avg;
        p = p + neg_lr * buf;
    } else {
        p = p + neg_lr * (g / avg);
    }
}

__global__ void __launch_bounds__(kT)
k_unet_rmsprop_step(const lnh_urs_tensor *__restrict__ table, uint32_t n, double *__restrict__ state, StepHyper h) {
    __shared__ uint32_t pre[65];
    const uint32_t total = table_prefix(table, n, pre);
    // read before block 0 writes anything: the slots written below are read by no workgroup
    const double sumsq = state[LNH_URS_SUMSQ], lr = state[LNH_URS_LR];
    const bool skip = state[LNH_URS_NONFINITE] != 0.0;
    const double norm = sqrt(sumsq) / h.loss_scale;
    const double c = h.max_norm / (norm + 1e-6);
    const float coef = (float)(c < 1.0 ? c : 1.0), neg_lr = -(float)lr;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[LNH_URS_NORM] = norm;
        state[LNH_URS_COEF] = (double)coef;
        if (skip) state[LNH_URS_SKIPPED] += 1.0;
        else state[LNH_URS_STEP] += 1.0;
    }
    if (skip) return;  // GradScaler.step on an inf: parameters and state keep every bit
    for (uint32_t ch = blockIdx.x; ch < total; ch += gridDim.x) {
        const uint32_t k = table_find(pre, ch);
        const lnh_urs_tensor T = table[k];
        const uint64_t off = (uint64_t)(ch - pre[k]) * kChunk, left = T.numel - off;
        const uint32_t m = left < kChunk ? (uint32_t)left : kChunk;
        float *p = T.param + off, *sq = T.square_avg + off, *buf = h.momentum > 0.0f ? T.momentum_buffer + off : nullptr;
        const float *g = T.grad + off;
        const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)sq) | ((uintptr_t)buf)) & 15) == 0;
        if (aligned) {
            float4 vp[4], vg[4], vs[4], vb[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t q = threadIdx.x + kT * j;
                if (4 * q + 3 < m) {
                    vp[j] = reinterpret_cast<const float4 *>(p)[q];
                    vg[j] = reinterpret_cast<const float4 *>(g)[q];
                    vs[j] = reinterpret_cast<const float4 *>(sq)[q];
                    vb[j] = buf ? reinterpret_cast<const float4 *>(buf)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t q = threadIdx.x + kT * j;
                if (4 * q + 3 < m) {
                    rmsprop_elem(vp[j].x, vg[j].x, vs[j].x, vb[j].x, h, coef, neg_lr);
                    rmsprop_elem(vp[j].y, vg[j].y, vs[j].y, vb[j].y, h, coef, neg_lr);
                    rmsprop_elem(vp[j].z, vg[j].z, vs[j].z, vb[j].z, h, coef, neg_lr);
                    rmsprop_elem(vp[j].w, vg[j].w, vs[j].w, vb[j].w, h, coef, neg_lr);
                    reinterpret_cast<float4 *>(p)[q] = vp[j];
                    reinterpret_cast<float4 *>(sq)[q] = vs[j];
                    if (buf) reinterpret_cast<float4 *>(buf)[q] = vb[j];
                }
            }
        }
        // the scalar path: everything of a tensor that does not start on 16 bytes, the last 1 .. 3 elements of any
        const uint32_t lo = aligned ? (m & ~3u) : 0u;
        for (uint32_t i = lo + threadIdx.x; i < m; i += kT) {
            float pv = p[i], sv = sq[i], bv = buf ? buf[i] : 0.f;
            rmsprop_elem(pv, g[i], sv, bv, h, coef, neg_lr);
            p[i] = pv;
            sq[i] = sv;
            if (buf) buf[i] = bv;
        }
    }
}

int check_table(const void *table, uint32_t n, const void *state, const char *who) {
    LNH_REQUIRE(table && state, LNH_ERR_INVALID_ARG, "%s: null pointer", who);
    LNH_REQUIRE(n >= 1 && n <= LNH_URS_MAX_TENSORS, LNH_ERR_INVALID_ARG, "%s: n_tensors %u; 1 .. %d tensors", who, n, LNH_URS_MAX_TENSORS);
    LNH_REQUIRE(((((uintptr_t)table) | ((uintptr_t)state)) & 7) == 0, LNH_ERR_INVALID_ARG, "%s: table and state must be 8-byte aligned", who);
    return LNH_OK;
}

}  // namespace

extern "C" {

uint64_t lnh_unet_loss_grad_workspace_size(uint64_t M) {
    if (M < 1 || M > kUnetMaxPixels) return 0;
    return (uint64_t)loss_parts(M) * 3 * sizeof(double);
}

int lnh_unet_loss_grad(const float *logits, const void *masks, uint32_t mask_dtype, uint64_t M, double loss_scale, void *ws,
                       uint64_t ws_bytes, float *loss, float *dlogits, lnh_stream_t stream) {
    LNH_REQUIRE(logits && masks && ws && loss && dlogits, LNH_ERR_INVALID_ARG, "unet_loss_grad: null pointer");
    LNH_REQUIRE(mask_dtype == LNH_UNET_MASK_F32 || mask_dtype == LNH_UNET_MASK_U8, LNH_ERR_INVALID_ARG,
                "unet_loss_grad: mask_dtype %u; LNH_UNET_MASK_F32 or LNH_UNET_MASK_U8", mask_dtype);
    LNH_REQUIRE(M >= 1 && M <= kUnetMaxPixels, LNH_ERR_INVALID_ARG, "unet_loss_grad: M = %llu; 1 .. 2^26 elements", (unsigned long long)M);
    LNH_REQUIRE(std::isfinite(loss_scale) && loss_scale > 0.0, LNH_ERR_INVALID_ARG, "unet_loss_grad: loss_scale must be positive and finite");
    LNH_REQUIRE(ws_bytes >= lnh_unet_loss_grad_workspace_size(M), LNH_ERR_INVALID_ARG, "unet_loss_grad: workspace of %llu bytes, %llu needed",
                (unsigned long long)ws_bytes, (unsigned long long)lnh_unet_loss_grad_workspace_size(M));
    LNH_REQUIRE(((((uintptr_t)logits) | ((uintptr_t)loss) | ((uintptr_t)dlogits)) & 3) == 0 && (((uintptr_t)ws) & 7) == 0 &&
                    (mask_dtype == LNH_UNET_MASK_U8 || (((uintptr_t)masks) & 3) == 0),
                LNH_ERR_INVALID_ARG, "unet_loss_grad: f32 buffers must be 4-byte aligned, the workspace 8-byte aligned");
    const uint64_t E = loss_block_elems(M);
    const uint32_t parts = loss_parts(M);
    hipStream_t s = (hipStream_t)stream;
    if (mask_dtype == LNH_UNET_MASK_U8) {
        LNH_LAUNCH(k_unet_loss_partials<true>, dim3(parts), dim3(kT), 0, s, logits, masks, M, E, (double *)ws);
        LNH_LAUNCH(k_unet_loss_grad<true>, dim3(parts), dim3(kT), 0, s, logits, masks, M, E, (const double *)ws, loss_scale, loss, dlogits);
    } else {
        LNH_LAUNCH(k_unet_loss_partials<false>, dim3(parts), dim3(kT), 0, s, logits, masks, M, E, (double *)ws);
        LNH_LAUNCH(k_unet_loss_grad<false>, dim3(parts), dim3(kT), 0, s, logits, masks, M, E, (const double *)ws, loss_scale, loss, dlogits);
    }
    return lnh_check_launch("lnh_unet_loss_grad");
}

uint64_t lnh_unet_grad_sumsq_workspace_size(void) { return (uint64_t)kSumBlocks * sizeof(double); }

int lnh_unet_grad_sumsq(const lnh_urs_tensor *table, uint32_t n_tensors, void *ws, uint64_t ws_bytes, double *state, lnh_stream_t stream) {
    if (int rc = check_table(table, n_tensors, state, "unet_grad_sumsq")) return rc;
    LNH_REQUIRE(ws && (((uintptr_t)ws) & 7) == 0, LNH_ERR_INVALID_ARG, "unet_grad_sumsq: the workspace must be a non-null 8-byte aligned pointer");
    LNH_REQUIRE(ws_bytes >= lnh_unet_grad_sumsq_workspace_size(), LNH_ERR_INVALID_ARG, "unet_grad_sumsq: workspace of %llu bytes, %llu needed",
                (unsigned long long)ws_bytes, (unsigned long long)lnh_unet_grad_sumsq_workspace_size());
    LNH_LAUNCH(k_unet_grad_sumsq, dim3(kSumBlocks), dim3(kT), 0, (hipStream_t)stream, table, n_tensors, (double *)ws);
    LNH_LAUNCH(k_unet_grad_sumsq_finish, dim3(1), dim3(kT), 0, (hipStream_t)stream, (const double *)ws, state);
    return lnh_check_launch("lnh_unet_grad_sumsq");
}

int lnh_unet_rmsprop_step(const lnh_urs_tensor *table, uint32_t n_tensors, double *state, double loss_scale, double max_norm,
                          double alpha, double eps, double weight_decay, double momentum, lnh_stream_t stream) {
    if (int rc = check_table(table, n_tensors, state, "unet_rmsprop_step")) return rc;
    LNH_REQUIRE(std::isfinite(loss_scale) && loss_scale > 0.0, LNH_ERR_INVALID_ARG, "unet_rmsprop_step: loss_scale must be positive and finite");
    LNH_REQUIRE(max_norm > 0.0, LNH_ERR_INVALID_ARG, "unet_rmsprop_step: max_norm must be positive (inf: no clipping)");
    LNH_REQUIRE(std::isfinite(alpha) && alpha >= 0.0, LNH_ERR_INVALID_ARG, "unet_rmsprop_step: alpha must be finite and >= 0");
    LNH_REQUIRE(std::isfinite(eps) && eps >= 0.0, LNH_ERR_INVALID_ARG, "unet_rmsprop_step: eps must be finite and >= 0");
    LNH_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.0, LNH_ERR_INVALID_ARG, "unet_rmsprop_step: weight_decay must be finite and >= 0");
    LNH_REQUIRE(std::isfinite(momentum) && momentum >= 0.0, LNH_ERR_INVALID_ARG, "unet_rmsprop_step: momentum must be finite and >= 0");
    StepHyper h;
    h.loss_scale = loss_scale;
    h.max_norm = max_norm;
    h.inv_scale = (float)(1.0 / loss_scale);
    h.alpha = (float)alpha;
    h.one_minus_alpha = (float)(1.0 - alpha);
    h.eps = (float)eps;
    h.wd = (float)weight_decay;
    h.momentum = (float)momentum;
    LNH_LAUNCH(k_unet_rmsprop_step, dim3(kStepBlocks), dim3(kT), 0, (hipStream_t)stream, table, n_tensors, state, h);
    return lnh_check_launch("lnh_unet_rmsprop_step");
}

}  // extern "C"
