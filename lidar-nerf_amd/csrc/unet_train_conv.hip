// unet_train_conv.hip — the training-mode convolution layer of the ray-drop U-Net around the raw convolution: weight
// pack, batch statistics, BatchNorm + ReLU and their backward.  Contract: include/lidarnerf_hip.h, "U-Net training".  (The raw
// convolution itself — lnh_unet_conv3x3_raw, forward and data gradient — is the RAW epilogue of k_unet_conv3x3 in unet.hip.)  The
// 16-byte load, aligned16, the pixel bound and the channel-range message are unet_common.h's; the partial rule (bn_split) is this file's.
//   k_unet_pack_conv3x3   the live fp32 parameter [Cout, Cin, 3, 3] -> the forward image [Cout, 9, Cpad] of lnh_unet_conv3x3 (thread
//                         per (co, padded ci), ci fastest: nine coalesced 2-byte stores) and the data-gradient image [Cin, 9, Cout],
//                         bwd[ci, t, co] = W[co, ci, 8 - t] (thread per (ci, co), co fastest).
//   k_unet_bn_stats       sum z and sum z^2 per channel in float64.  A workgroup owns 64 channels of the P pixels of one partial; a thread
//                         owns 8 of them (one 16-byte read per pixel) and row r of the workgroup's 32 rows: it chains the pixels begin + r,
//                         begin + r + 32, ..; the 32 rows are then added per channel in ascending r (through LDS, plain stores and
//                         loads) and the workgroup's partial goes to the workspace.  k_unet_bn_stats_finish adds the partials in ascending order
//                         and forms mean, var, invstd, scale, shift and the running statistics in float64, each rounded once.
//   k_unet_bn_relu        a = fp16(max(fmaf(float(z), scale, shift), 0)), 8 channels per thread.
//   k_unet_bn_bwd_sums    dbeta = sum g, dgamma = sum g xhat with g = da [a > 0], xhat = (float(z) - mean) invstd and the product in fp32;
//                         the same ownership and order of addition as k_unet_bn_stats, in float64.  k_unet_bn_bwd_finish rounds the
//                         two sums to f32.
//   k_unet_bn_bwd_dz      dz = fp16(scale (g - dbeta / M - xhat dgamma / M)) in fp32; every element is read before its owner writes it,
//                         so dz may be da.
#include "unet_common.h"

namespace {

constexpr uint32_t kBnBlockPixels = 256;    // pixels per partial, times ceil(M / 2^14): at most 64 partials per channel
constexpr uint64_t kBnPartialSpan = 1ull << 14;
constexpr uint32_t kBnSlab = 64, kBnRows = 32;  // channels per workgroup; pixel rows of its 256 threads

struct PackConvArgs {
    const float *w;
    half_t *fwd, *bwd;
    uint32_t Cout, Cin, Cpad;
};

__global__ void __launch_bounds__(256)
k_unet_pack_conv3x3(PackConvArgs a) {
    const uint64_t nf = (uint64_t)a.Cout * a.Cpad, nb = a.bwd ? (uint64_t)a.Cin * a.Cout : 0;
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nf) {  // forward image [co][t][ci]
        const uint32_t ci = (uint32_t)(i % a.Cpad), co = (uint32_t)(i / a.Cpad);
        const float *src = a.w + ((uint64_t)co * a.Cin + ci) * 9;
#pragma unroll
        for (uint32_t t = 0; t < 9; t++) a.fwd[((uint64_t)co * 9 + t) * a.Cpad + ci] = ci < a.Cin ? (half_t)src[t] : (half_t)0;
        return;
    }
    i -= nf;
    if (i >= nb) return;
    const uint32_t co = (uint32_t)(i % a.Cout), ci = (uint32_t)(i / a.Cout);  // data-gradient image [ci][t][co]
    const float *src = a.w + ((uint64_t)co * a.Cin + ci) * 9;
#pragma unroll
    for (uint32_t t = 0; t < 9; t++) a.bwd[((uint64_t)ci * 9 + t) * a.Cout + co] = (half_t)src[8 - t];
}

// The cut of M pixels into partials, from the shape alone.
struct BnSplit {
    uint32_t P, parts;
};

BnSplit bn_split(uint64_t M) {
    const uint32_t P = kBnBlockPixels * (uint32_t)((M + kBnPartialSpan - 1) / kBnPartialSpan);
    return BnSplit{P, (uint32_t)((M + P - 1) / P)};
}

bool bn_shape_ok(uint64_t M, uint32_t C) { return M >= 2 && M <= kUnetMaxPixels && unet_channels_ok(C, 32); }

// A workgroup owns kBnSlab channels (slab blockIdx.y) of the P pixels of partial blockIdx.x: thread (r, g) = (t / 8, t % 8) chains 8
// channels over the pixels begin + r, begin + r + 32, ..  This adds the 32 rows per column in ascending r and writes the partial.
__device__ __forceinline__ void bn_block_partial(const double (&s0)[8], const double (&s1)[8], uint32_t C, double *part) {
    __shared__ double rows[kBnRows * 2 * kBnSlab];  // [r][which][channel of the slab]
    const uint32_t g = threadIdx.x % 8, r = threadIdx.x / 8;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        rows[(r * 2 + 0) * kBnSlab + 8 * g + j] = s0[j];
        rows[(r * 2 + 1) * kBnSlab + 8 * g + j] = s1[j];
    }
    __syncthreads();
    if (threadIdx.x >= 2 * kBnSlab) return;
    const uint32_t which = threadIdx.x / kBnSlab, j = threadIdx.x % kBnSlab, c = blockIdx.y * kBnSlab + j;
    if (c >= C) return;  // (C = 96, 160, ..: the last slab is half used)
    double s = 0.0;
    for (uint32_t k = 0; k < kBnRows; k++) s += rows[(k * 2 + which) * kBnSlab + j];
    part[((uint64_t)blockIdx.x * 2 + which) * C + c] = s;
}

struct BnStatsArgs {
    const half_t *z;
    double *part;  // [parts][2][C]
    uint32_t C, P;
    uint64_t M;
};

__global__ void __launch_bounds__(256)
k_unet_bn_stats(BnStatsArgs a) {
    const uint32_t g = threadIdx.x % 8, r = threadIdx.x / 8, c0 = blockIdx.y * kBnSlab + 8 * g;
    const uint64_t begin = (uint64_t)blockIdx.x * a.P, end = begin + a.P < a.M ? begin + a.P : a.M;
    double s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s0[j] = s1[j] = 0.0;
#pragma unroll 4
    for (uint64_t p = c0 < a.C ? begin + r : end; p < end; p += kBnRows) {
        const half8_t v = ld8(a.z + p * a.C + c0);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double x = (double)v[j];
            s0[j] += x;
            s1[j] += x * x;  // (exact: an fp16 square has 22 bits)
        }
    }
    bn_block_partial(s0, s1, a.C, a.part);
}

struct BnFinishArgs {
    const double *part;
    const float *gamma, *beta;
    float *mean, *invstd, *scale, *shift, *running_mean, *running_var;
    double eps, momentum;
    uint32_t C, parts;
    uint64_t M;
};

__global__ void __launch_bounds__(256)
k_unet_bn_stats_finish(BnFinishArgs a) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (uint32_t k = 0; k < a.parts; k++) {
        s0 += a.part[(uint64_t)k * 2 * a.C + c];
        s1 += a.part[(uint64_t)k * 2 * a.C + a.C + c];
    }
    const double M = (double)a.M, mean = s0 / M;
    double var = s1 / M - mean * mean;
    if (var < 0.0) var = 0.0;  // (not fmax: a NaN stays a NaN)
    const double invstd = 1.0 / sqrt(var + a.eps), scale = (double)a.gamma[c] * invstd;
    a.mean[c] = (float)mean;
    a.invstd[c] = (float)invstd;
    a.scale[c] = (float)scale;
    a.shift[c] = (float)((double)a.beta[c] - mean * scale);
    if (a.running_mean) a.running_mean[c] = (float)((1.0 - a.momentum) * (double)a.running_mean[c] + a.momentum * mean);
    if (a.running_var) a.running_var[c] = (float)((1.0 - a.momentum) * (double)a.running_var[c] + a.momentum * (var * (M / (M - 1.0))));
}

struct BnReluArgs {
    const half_t *z;
    const float *scale, *shift;
    half_t *a;
    uint32_t C;
    uint64_t M;
};

__global__ void __launch_bounds__(256)
k_unet_bn_relu(BnReluArgs a) {
    const uint32_t G = a.C / 8;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M * G) return;
    const uint32_t c0 = (uint32_t)(i % G) * 8;
    const half8_t v = ld8(a.z + i * 8);
    const f32x4 s[2] = {*reinterpret_cast<const f32x4 *>(a.scale + c0), *reinterpret_cast<const f32x4 *>(a.scale + c0 + 4)};
    const f32x4 t[2] = {*reinterpret_cast<const f32x4 *>(a.shift + c0), *reinterpret_cast<const f32x4 *>(a.shift + c0 + 4)};
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = (half_t)fmaxf(fmaf((float)v[j], s[j >> 2][j & 3], t[j >> 2][j & 3]), 0.0f);
    *reinterpret_cast<half8_t *>(a.a + i * 8) = o;
}

struct BnBwdArgs {
    const half_t *z, *a, *da;
    const float *mean, *invstd, *scale, *dgamma, *dbeta;
    half_t *dz;
    double *part;  // [parts][2][C]: dbeta, dgamma
    uint32_t C, P;
    uint64_t M;
};

__global__ void __launch_bounds__(256)
k_unet_bn_bwd_sums(BnBwdArgs a) {
    const uint32_t g = threadIdx.x % 8, r = threadIdx.x / 8, c0 = blockIdx.y * kBnSlab + 8 * g;
    const bool live = c0 < a.C;
    const uint64_t begin = (uint64_t)blockIdx.x * a.P, end = begin + a.P < a.M ? begin + a.P : a.M;
    float mu[8], is[8];
#pragma unroll
    for (int j = 0; j < 8; j++) mu[j] = live ? a.mean[c0 + j] : 0.0f, is[j] = live ? a.invstd[c0 + j] : 0.0f;
    double s0[8], s1[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s0[j] = s1[j] = 0.0;
#pragma unroll 2
    for (uint64_t p = live ? begin + r : end; p < end; p += kBnRows) {
        const uint64_t e = p * a.C + c0;
        const half8_t z = ld8(a.z + e), act = ld8(a.a + e), da = ld8(a.da + e);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float gj = act[j] > (half_t)0 ? (float)da[j] : 0.0f;
            const float xh = ((float)z[j] - mu[j]) * is[j];
            s0[j] += (double)gj;
            s1[j] += (double)(gj * xh);
        }
    }
    bn_block_partial(s0, s1, a.C, a.part);
}

__global__ void __launch_bounds__(256)
k_unet_bn_bwd_finish(const double *__restrict__ part, uint32_t parts, uint32_t C, float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (uint32_t k = 0; k < parts; k++) {
        s0 += part[(uint64_t)k * 2 * C + c];
        s1 += part[(uint64_t)k * 2 * C + C + c];
    }
    dbeta[c] = (float)s0;
    dgamma[c] = (float)s1;
}

__global__ void __launch_bounds__(256)
k_unet_bn_bwd_dz(BnBwdArgs a) {
    const uint32_t G = a.C / 8;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M * G) return;
    const uint32_t c0 = (uint32_t)(i % G) * 8;
    const half8_t z = ld8(a.z + i * 8), act = ld8(a.a + i * 8), da = ld8(a.da + i * 8);
    const float M = (float)a.M;
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t c = c0 + j;
        const float gj = act[j] > (half_t)0 ? (float)da[j] : 0.0f;
        const float xh = ((float)z[j] - a.mean[c]) * a.invstd[c];
        o[j] = (half_t)(a.scale[c] * ((gj - a.dbeta[c] / M) - xh * (a.dgamma[c] / M)));
    }
    *reinterpret_cast<half8_t *>(a.dz + i * 8) = o;
}

}  // namespace

extern "C" {

int lnh_unet_pack_conv3x3(const float *weight, uint32_t Cout, uint32_t Cin, void *fwd, void *bwd, lnh_stream_t stream) {
    LNH_REQUIRE(weight && fwd, LNH_ERR_INVALID_ARG, "unet_pack_conv3x3: null pointer");
    UNET_REQUIRE_CHANNELS("unet_pack_conv3x3", "Cout", Cout, 64);
    LNH_REQUIRE(Cin >= 1 && Cin <= 1024 && (Cin <= 32 || Cin % 32 == 0), LNH_ERR_INVALID_ARG,
                "unet_pack_conv3x3: Cin %u (1 .. 32, or a multiple of 32 up to 1024)", Cin);
    LNH_REQUIRE(!bwd || Cin % 64 == 0, LNH_ERR_INVALID_ARG, "unet_pack_conv3x3: the bwd image needs Cin %u to be a multiple of 64", Cin);
    LNH_REQUIRE(aligned16(weight) && aligned16(fwd) && aligned16(bwd), LNH_ERR_INVALID_ARG, "unet_pack_conv3x3: every pointer must be 16-byte aligned");
    PackConvArgs a{weight, (half_t *)fwd, (half_t *)bwd, Cout, Cin, Cin <= 32 ? 32u : Cin};
    const uint64_t threads = (uint64_t)Cout * a.Cpad + (bwd ? (uint64_t)Cin * Cout : 0);
    LNH_LAUNCH(k_unet_pack_conv3x3, dim3(div_up(threads, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_pack_conv3x3");
}

uint64_t lnh_unet_bn_stats_workspace_size(uint64_t M, uint32_t C) {
    if (!bn_shape_ok(M, C)) return 0;
    return (uint64_t)bn_split(M).parts * 2 * C * sizeof(double);
}

int lnh_unet_bn_stats(const void *z, uint64_t M, uint32_t C, const float *gamma, const float *beta, double eps, double momentum,
                      void *ws, uint64_t ws_bytes, float *mean, float *invstd, float *scale, float *shift, float *running_mean,
                      float *running_var, lnh_stream_t stream) {
    LNH_REQUIRE(z && gamma && beta && ws && mean && invstd && scale && shift, LNH_ERR_INVALID_ARG, "unet_bn_stats: null pointer");
    LNH_REQUIRE(M >= 2 && M <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "unet_bn_stats: M %llu values per channel (2 .. 2^26; one value has no variance)", (unsigned long long)M);
    UNET_REQUIRE_CHANNELS("unet_bn_stats", "C", C, 32);
    LNH_REQUIRE(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, LNH_ERR_INVALID_ARG,
                "unet_bn_stats: eps %g (>= 0), momentum %g (0 .. 1)", eps, momentum);
    const uint64_t need = lnh_unet_bn_stats_workspace_size(M, C);
    LNH_REQUIRE(ws_bytes >= need, LNH_ERR_INVALID_ARG, "unet_bn_stats: workspace of %llu bytes, %llu needed",
                (unsigned long long)ws_bytes, (unsigned long long)need);
    LNH_REQUIRE(aligned16(z) && aligned16(ws) && aligned16(scale) && aligned16(shift), LNH_ERR_INVALID_ARG,
                "unet_bn_stats: z, the workspace, scale and shift must be 16-byte aligned");
    const BnSplit sp = bn_split(M);
    const hipStream_t s = (hipStream_t)stream;
    BnStatsArgs a{(const half_t *)z, (double *)ws, C, sp.P, M};
    LNH_LAUNCH(k_unet_bn_stats, dim3(sp.parts, div_up(C, kBnSlab)), dim3(256), 0, s, a);
    BnFinishArgs f{(const double *)ws, gamma, beta, mean, invstd, scale, shift, running_mean, running_var, eps, momentum, C, sp.parts, M};
    LNH_LAUNCH(k_unet_bn_stats_finish, dim3(div_up(C, 256)), dim3(256), 0, s, f);
    return lnh_check_launch("lnh_unet_bn_stats");
}

int lnh_unet_bn_relu(const void *z, uint64_t M, uint32_t C, const float *scale, const float *shift, void *a, lnh_stream_t stream) {
    LNH_REQUIRE(z && scale && shift && a, LNH_ERR_INVALID_ARG, "unet_bn_relu: null pointer");
    LNH_REQUIRE(M >= 1 && M <= kUnetMaxPixels, LNH_ERR_INVALID_ARG, "unet_bn_relu: M %llu pixels (1 .. 2^26)", (unsigned long long)M);
    UNET_REQUIRE_CHANNELS("unet_bn_relu", "C", C, 32);
    LNH_REQUIRE(aligned16(z) && aligned16(scale) && aligned16(shift) && aligned16(a), LNH_ERR_INVALID_ARG,
                "unet_bn_relu: every pointer must be 16-byte aligned");
    BnReluArgs r{(const half_t *)z, scale, shift, (half_t *)a, C, M};
    LNH_LAUNCH(k_unet_bn_relu, dim3(div_up(M * (C / 8), 256)), dim3(256), 0, (hipStream_t)stream, r);
    return lnh_check_launch("lnh_unet_bn_relu");
}

uint64_t lnh_unet_bn_relu_backward_workspace_size(uint64_t M, uint32_t C) { return lnh_unet_bn_stats_workspace_size(M, C); }

int lnh_unet_bn_relu_backward(const void *z, const void *a, const void *da, uint64_t M, uint32_t C, const float *mean,
                              const float *invstd, const float *scale, void *ws, uint64_t ws_bytes, void *dz, float *dgamma,
                              float *dbeta, lnh_stream_t stream) {
    LNH_REQUIRE(z && a && da && mean && invstd && scale && ws && dz && dgamma && dbeta, LNH_ERR_INVALID_ARG,
                "unet_bn_relu_backward: null pointer");
    LNH_REQUIRE(M >= 2 && M <= kUnetMaxPixels, LNH_ERR_INVALID_ARG, "unet_bn_relu_backward: M %llu values per channel (2 .. 2^26)",
                (unsigned long long)M);
    UNET_REQUIRE_CHANNELS("unet_bn_relu_backward", "C", C, 32);
    const uint64_t need = lnh_unet_bn_relu_backward_workspace_size(M, C);
    LNH_REQUIRE(ws_bytes >= need, LNH_ERR_INVALID_ARG, "unet_bn_relu_backward: workspace of %llu bytes, %llu needed",
                (unsigned long long)ws_bytes, (unsigned long long)need);
    LNH_REQUIRE(aligned16(z) && aligned16(a) && aligned16(da) && aligned16(ws) && aligned16(dz), LNH_ERR_INVALID_ARG,
                "unet_bn_relu_backward: z, a, da, the workspace and dz must be 16-byte aligned");
    const BnSplit sp = bn_split(M);
    const hipStream_t s = (hipStream_t)stream;
    BnBwdArgs b{(const half_t *)z, (const half_t *)a, (const half_t *)da, mean, invstd, scale, dgamma, dbeta, (half_t *)dz, (double *)ws,
                C, sp.P, M};
    LNH_LAUNCH(k_unet_bn_bwd_sums, dim3(sp.parts, div_up(C, kBnSlab)), dim3(256), 0, s, b);
    LNH_LAUNCH(k_unet_bn_bwd_finish, dim3(div_up(C, 256)), dim3(256), 0, s, (const double *)ws, sp.parts, C, dgamma, dbeta);
    LNH_LAUNCH(k_unet_bn_bwd_dz, dim3(div_up(M * (C / 8), 256)), dim3(256), 0, s, b);
    return lnh_check_launch("lnh_unet_bn_relu_backward");
}

}  // extern "C"
