// unet_train.hip — backward kernels of the ray-drop U-Net's training step: the max-pool backward with the skip add, the
// backward of the 1 x 1 head, the transposed convolution's weight pack and data gradient.  Contract: include/lidarnerf_hip.h,
// "U-Net training".  unet_common.h: the small helpers, the dy window both transposed-convolution entry points require
// (unet_upconv_dy_window), the channel-range message and the slice split of the weight gradient (unet_pixel_split).
//   k_unet_pool_backward  one thread owns 8 channels of one source pixel: it re-reads its 2 x 2 window, finds the first maximum in
//                         row-major order (strict >, and a NaN takes over: torch's rule) and takes the pooled gradient if that is its own position; the
//                         skip gradient — channels [0, C) of a wider tensor, read in place through a pixel stride — is added in fp32
//                         and the sum rounded once.  One owner per element, no atomics.
//   k_unet_head_backward  one thread per pixel: dx[p, c] = fp16(dlogit[p] w[c]); the 64 products dlogit[p] a[p, c] and dlogit[p] are
//                         added over the wave's 64 pixels by the xor butterfly (offsets 32, 16, .., 1) in fp32 and lane 0 writes the
//                         65 partials of the wave to the workspace.
//   k_unet_head_finish    thread c adds the waves' partials of column c in ascending order in float64: dweight[c], dbias.
//   k_unet_pack_upconv    the transposed convolution's fp32 parameter [Cin, Cout, 2, 2] -> the forward image [4, Cout, Cin] of
//                         lnh_unet_upconv2x2 and the data-gradient image [Cin, 4, Cout], both fp16.
//   k_unet_upconv_bwd_data  dx[p, ci] = sum_{q, co} dy[2p + q, co] W[ci, co, q] on v_mfma_f32_16x16x32_f16, the product of
//                         k_unet_upconv with the roles turned: rows ci, k = (q, co).  A wave owns 16 input pixels x 64 ci; the A
//                         operand is 8 consecutive fp16 of one image row, the B operand 8 consecutive channels of output pixel
//                         2p + q — read in place from the concatenation's gradient tensor (pixel stride, channel offset, its own
//                         height and width: the crop of the padded row / column costs nothing).
//   k_unet_upconv_bwd_weight  dW[ci, co, q] = sum_p x[p, ci] dy[2p + q, co], dbias[co] = sum dy.  The summed index (the pixel) is the
//                         slow memory index of both operands, so a workgroup stages 32 pixels x 64 ci of x and, per q, 32 pixels x 64
//                         co of dy in LDS with 16-byte reads (a pixel past the slice is zero-filled, never branched on) and every lane
//                         gathers its 8 k-values with 16-bit LDS reads; k = 8 g + j of an MFMA is tile row 4 j + g, which with the row
//                         pitch of 80 halves puts the 32 lanes of an LDS cycle on 16 distinct banks.  Wave w owns the co 16 w .. 16 w
//                         + 15 of the block, all 64 ci and the four q (16 accumulators).  Workgroup (slice, ci block, co block) sums
//                         the pixels of its slice in steps of 32 and writes its partial to the workspace in the parameter's
//                         [Cin, Cout, 2, 2] layout; the workgroups of ci block 0 also add the dy tiles per co (q, then tile row,
//                         ascending, one fp32 chain).  k_unet_upconv_bwd_reduce adds the slices in ascending order in float64.
#include "unet_common.h"

namespace {

constexpr uint32_t kHeadC = 64, kHeadCols = kHeadC + 1;  // the head's input channels; + 1 column for the bias

struct PoolBwdArgs {
    const half_t *x, *dpool, *dskip;
    half_t *dx;
    uint32_t H0, W0, C, skip_stride;
    uint64_t M0;  // N H0 W0
};

__global__ void __launch_bounds__(256)
k_unet_pool_backward(PoolBwdArgs a) {
    const uint32_t groups = a.C / 8;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M0 * groups) return;
    const uint64_t p = i / groups;
    const uint32_t c0 = (uint32_t)(i % groups) * 8;
    const UnetPixel s = unet_pixel(p, a.H0, a.W0);
    const uint32_t n = s.n, y = s.y, x = s.x, H = a.H0 / 2, W = a.W0 / 2, py = y / 2, px = x / 2;
    float out[8];
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = 0.0f;
    if (py < H && px < W) {  // (a last odd row or column belongs to no window)
        const half_t *win = a.x + (((uint64_t)n * a.H0 + 2 * py) * a.W0 + 2 * px) * a.C + c0;
        const uint64_t row = (uint64_t)a.W0 * a.C;
        const half8_t v[4] = {ld8(win), ld8(win + a.C), ld8(win + row), ld8(win + row + a.C)};
        const half8_t d = ld8(a.dpool + (((uint64_t)n * H + py) * W + px) * a.C + c0);
        const int mine = (int)((y & 1) * 2 + (x & 1));
#pragma unroll
        for (int j = 0; j < 8; j++) {
            int first = 0;
            half_t best = v[0][j];
#pragma unroll
            for (int k = 1; k < 4; k++)
                if (v[k][j] > best || v[k][j] != v[k][j]) best = v[k][j], first = k;  // (a NaN takes over, as in torch)
            if (first == mine) out[j] = (float)d[j];
        }
    }
    if (a.dskip) {
        const half8_t s = ld8(a.dskip + p * a.skip_stride + c0);
#pragma unroll
        for (int j = 0; j < 8; j++) out[j] += (float)s[j];
    }
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = (half_t)out[j];
    *reinterpret_cast<half8_t *>(a.dx + p * a.C + c0) = o;
}

struct HeadBwdArgs {
    const half_t *a, *w;
    const float *dlogits;
    half_t *dx;
    float *part;  // [waves][65]
    uint64_t M;
};

__global__ void __launch_bounds__(256)
k_unet_head_backward(HeadBwdArgs a) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < a.M;  // (no early return: the whole wave takes part in the butterfly)
    const float d = valid ? a.dlogits[p] : 0.0f;
    const uint64_t wave = p >> 6;
    const bool writer = (threadIdx.x & 63) == 0 && valid;  // (lane 0 is valid whenever any lane of its wave is)
#pragma unroll
    for (uint32_t k = 0; k < kHeadC / 8; k++) {
        const half8_t w = ld8(a.w + 8 * k);
        half8_t x = zero8(), o;
        if (valid) x = ld8(a.a + p * kHeadC + 8 * k);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            o[j] = (half_t)(d * (float)w[j]);
            const float s = wave_sum(valid ? d * (float)x[j] : 0.0f);
            if (writer) a.part[wave * kHeadCols + 8 * k + j] = s;
        }
        if (valid) *reinterpret_cast<half8_t *>(a.dx + p * kHeadC + 8 * k) = o;
    }
    const float s = wave_sum(d);
    if (writer) a.part[wave * kHeadCols + kHeadC] = s;
}

__global__ void __launch_bounds__(128)
k_unet_head_finish(const float *__restrict__ part, uint64_t waves, float *__restrict__ dweight, float *__restrict__ dbias) {
    const uint32_t c = threadIdx.x;
    if (c >= kHeadCols) return;
    double s = 0.0;
    for (uint64_t k = 0; k < waves; k++) s += (double)part[k * kHeadCols + c];
    if (c < kHeadC) dweight[c] = (float)s;
    else dbias[0] = (float)s;
}

struct PackUpArgs {
    const float *w;
    half_t *fwd, *bwd;
    uint32_t Cin, Cout;
};

__global__ void __launch_bounds__(256)
k_unet_pack_upconv(PackUpArgs a) {
    const uint64_t n = (uint64_t)a.Cin * a.Cout * 4;
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {  // forward image [q][co][ci]
        const uint32_t ci = (uint32_t)(i % a.Cin), co = (uint32_t)(i / a.Cin % a.Cout), q = (uint32_t)(i / a.Cin / a.Cout);
        a.fwd[i] = (half_t)a.w[((uint64_t)ci * a.Cout + co) * 4 + q];
        return;
    }
    i -= n;
    if (i >= n || !a.bwd) return;
    const uint32_t co = (uint32_t)(i % a.Cout), q = (uint32_t)(i / a.Cout % 4), ci = (uint32_t)(i / a.Cout / 4);  // [ci][q][co]
    a.bwd[i] = (half_t)a.w[((uint64_t)ci * a.Cout + co) * 4 + q];
}

struct UpBwdArgs {
    const half_t *dy, *w;
    half_t *dx;
    uint32_t H, W, Hd, Wd, stride, off, Cin, Cout;
    uint64_t M;  // N H W of the input
};

__global__ void __launch_bounds__(256)
k_unet_upconv_bwd_data(UpBwdArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const uint64_t base = ((uint64_t)blockIdx.x * 4 + wave) * 16;
    if (base >= a.M) return;  // (no barrier in this kernel)
    const uint32_t ci0 = blockIdx.y * 64;
    const uint64_t p = base + c;
    const bool valid = p < a.M;
    const UnetPixel s = unet_pixel(valid ? p : 0, a.H, a.W);
    const uint32_t n = s.n, y = s.y, x = s.x;
    const half_t *wrow[4];
#pragma unroll
    for (int t = 0; t < 4; t++) wrow[t] = a.w + (uint64_t)(ci0 + 16 * t + c) * 4 * a.Cout + 8 * g;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
    for (uint32_t q = 0; q < 4; q++) {
        const half_t *src = a.dy + (((uint64_t)n * a.Hd + 2 * y + (q >> 1)) * a.Wd + 2 * x + (q & 1)) * a.stride + a.off + 8 * g;
#pragma unroll 2
        for (uint32_t ch = 0; ch < a.Cout; ch += 32) {
            half8_t wf[4];
#pragma unroll
            for (int t = 0; t < 4; t++) wf[t] = ld8(wrow[t] + q * a.Cout + ch);
            const half8_t df = valid ? ld8(src + ch) : zero8();
#pragma unroll
            for (int t = 0; t < 4; t++) acc[t] = UNET_MFMA(wf[t], df, acc[t]);
        }
    }
    if (!valid) return;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        half4_t o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = (half_t)acc[t][r];
        *reinterpret_cast<half4_t *>(a.dx + p * a.Cin + ci0 + 16 * t + 4 * g) = o;
    }
}

constexpr uint32_t kUpPitch = 80;                 // halves per LDS row of 64 channels
constexpr uint64_t kUpSliceBudget = 16ull << 20;  // bytes of slices the split rule allows itself

struct UpWgtArgs {
    const half_t *x, *dy;
    float *part;  // [S][Cin Cout 4 + Cout]
    uint32_t H, W, Hd, Wd, stride, off, Cin, Cout;
    uint64_t M, L;  // input pixels; pixels per slice (a multiple of 32)
};

__global__ void __launch_bounds__(256)
k_unet_upconv_bwd_weight(UpWgtArgs a) {
    __shared__ __attribute__((aligned(16))) half_t xs[32][kUpPitch];
    __shared__ __attribute__((aligned(16))) half_t ds[4][32][kUpPitch];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, c = lane & 15, g = lane >> 4;
    const uint32_t spix = t >> 3, chunk = t & 7;  // this thread's tile row and 8-channel chunk when staging
    const uint32_t ci0 = blockIdx.y * 64, co0 = blockIdx.z * 64;
    const uint64_t begin = (uint64_t)blockIdx.x * a.L, end = begin + a.L < a.M ? begin + a.L : a.M;
    const bool bias_owner = blockIdx.y == 0 && t < 64;
    float bias = 0.0f;
    f32x4 acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[q][i] = f32x4{0, 0, 0, 0};

    for (uint64_t base = begin; base < end; base += 32) {
        const uint64_t p = base + spix;
        const bool valid = p < end;
        const UnetPixel s = unet_pixel(valid ? p : 0, a.H, a.W);
        const uint32_t n = s.n, y = s.y, x = s.x;
        *reinterpret_cast<half8_t *>(&xs[spix][8 * chunk]) = valid ? ld8(a.x + p * a.Cin + ci0 + 8 * chunk) : zero8();
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const half_t *src = a.dy + (((uint64_t)n * a.Hd + 2 * y + (q >> 1)) * a.Wd + 2 * x + (q & 1)) * a.stride + a.off + co0 + 8 * chunk;
            *reinterpret_cast<half8_t *>(&ds[q][spix][8 * chunk]) = valid ? ld8(src) : zero8();
        }
        __syncthreads();
        half8_t af[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 8; j++) af[i][j] = xs[4 * j + g][16 * i + c];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            half8_t bf;
#pragma unroll
            for (int j = 0; j < 8; j++) bf[j] = ds[q][4 * j + g][16 * wave + c];
#pragma unroll
            for (int i = 0; i < 4; i++) acc[q][i] = UNET_MFMA(af[i], bf, acc[q][i]);
        }
        if (bias_owner) {
            for (int q = 0; q < 4; q++)
                for (int r = 0; r < 32; r++) bias += (float)ds[q][r][t];
        }
        __syncthreads();
    }
    const uint64_t slice = (uint64_t)a.Cin * a.Cout * 4 + a.Cout;
    float *dst = a.part + (uint64_t)blockIdx.x * slice;
    const uint32_t co = co0 + 16 * wave + c;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) dst[((uint64_t)(ci0 + 16 * i + 4 * g + r) * a.Cout + co) * 4 + q] = acc[q][i][r];
    if (bias_owner) dst[(uint64_t)a.Cin * a.Cout * 4 + co0 + t] = bias;
}

__global__ void __launch_bounds__(256)
k_unet_upconv_bwd_reduce(const float *__restrict__ part, uint32_t S, uint64_t nw, uint64_t slice, float *__restrict__ dweight,
                         float *__restrict__ dbias) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slice) return;
    double s = 0.0;
    for (uint32_t k = 0; k < S; k++) s += (double)part[(uint64_t)k * slice + i];
    if (i < nw) dweight[i] = (float)s;
    else dbias[i - nw] = (float)s;
}

// (the bias row of a slice is not counted against the 16 MiB)
UnetSplit upconv_wgrad_split(uint64_t M, uint32_t Cin, uint32_t Cout) { return unet_pixel_split(M, 16ull * Cin * Cout, kUpSliceBudget); }

bool upconv_wgrad_shape_ok(uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout) {
    return N && H && W && (uint64_t)N * H * W * 4 <= kUnetMaxPixels && unet_channels_ok(Cin, 64) && unet_channels_ok(Cout, 64);
}

}  // namespace

extern "C" {

int lnh_unet_pool_backward(const void *x, uint32_t N, uint32_t H0, uint32_t W0, uint32_t C, const void *dpool, const void *dskip,
                           uint32_t skip_stride, void *dx, lnh_stream_t stream) {
    LNH_REQUIRE(x && dpool && dx, LNH_ERR_INVALID_ARG, "unet_pool_backward: null pointer");
    UNET_REQUIRE_CHANNELS("unet_pool_backward", "C", C, 32);
    LNH_REQUIRE(N && H0 >= 2 && W0 >= 2 && (uint64_t)N * H0 * W0 <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "unet_pool_backward: source [%u, %u, %u] (at least 2 x 2, up to 2^26 pixels)", N, H0, W0);
    LNH_REQUIRE(dskip ? (skip_stride >= C && skip_stride <= 2048 && skip_stride % 8 == 0) : skip_stride == 0, LNH_ERR_INVALID_ARG,
                "unet_pool_backward: skip stride %u (with dskip: a multiple of 8 from C = %u to 2048; without: 0)", skip_stride, C);
    LNH_REQUIRE(aligned16(x) && aligned16(dpool) && aligned16(dskip) && aligned16(dx), LNH_ERR_INVALID_ARG,
                "unet_pool_backward: every pointer must be 16-byte aligned");
    PoolBwdArgs a{(const half_t *)x, (const half_t *)dpool, (const half_t *)dskip, (half_t *)dx, H0, W0, C, skip_stride,
                  (uint64_t)N * H0 * W0};
    LNH_LAUNCH(k_unet_pool_backward, dim3(div_up(a.M0 * (C / 8), 256)), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_pool_backward");
}

uint64_t lnh_unet_head_backward_workspace_size(uint32_t N, uint32_t H, uint32_t W) {
    const uint64_t M = (uint64_t)N * H * W;
    if (!N || !H || !W || M > kUnetMaxPixels) return 0;
    return (M + 63) / 64 * kHeadCols * sizeof(float);
}

int lnh_unet_head_backward(const void *a, uint32_t N, uint32_t H, uint32_t W, const void *weight, const float *dlogits, void *ws,
                           uint64_t ws_bytes, void *dx, float *dweight, float *dbias, lnh_stream_t stream) {
    LNH_REQUIRE(a && weight && dlogits && ws && dx && dweight && dbias, LNH_ERR_INVALID_ARG, "unet_head_backward: null pointer");
    const uint64_t need = lnh_unet_head_backward_workspace_size(N, H, W);
    LNH_REQUIRE(need, LNH_ERR_INVALID_ARG, "unet_head_backward: image [%u, %u, %u] (1 .. 2^26 pixels)", N, H, W);
    LNH_REQUIRE(ws_bytes >= need, LNH_ERR_INVALID_ARG, "unet_head_backward: workspace of %llu bytes, %llu needed",
                (unsigned long long)ws_bytes, (unsigned long long)need);
    LNH_REQUIRE(aligned16(a) && aligned16(weight) && aligned16(ws) && aligned16(dx), LNH_ERR_INVALID_ARG,
                "unet_head_backward: a, weight, the workspace and dx must be 16-byte aligned");
    const uint64_t M = (uint64_t)N * H * W;
    HeadBwdArgs h{(const half_t *)a, (const half_t *)weight, dlogits, (half_t *)dx, (float *)ws, M};
    LNH_LAUNCH(k_unet_head_backward, dim3(div_up(M, 256)), dim3(256), 0, (hipStream_t)stream, h);
    LNH_LAUNCH(k_unet_head_finish, dim3(1), dim3(128), 0, (hipStream_t)stream, (const float *)ws, (M + 63) / 64, dweight, dbias);
    return lnh_check_launch("lnh_unet_head_backward");
}

int lnh_unet_pack_upconv(const float *weight, uint32_t Cin, uint32_t Cout, void *fwd, void *bwd, lnh_stream_t stream) {
    LNH_REQUIRE(weight && fwd, LNH_ERR_INVALID_ARG, "unet_pack_upconv: null pointer");
    UNET_REQUIRE_CHANNELS("unet_pack_upconv", "Cin", Cin, 64);
    UNET_REQUIRE_CHANNELS("unet_pack_upconv", "Cout", Cout, 64);
    LNH_REQUIRE(aligned16(weight) && aligned16(fwd) && aligned16(bwd), LNH_ERR_INVALID_ARG,
                "unet_pack_upconv: every pointer must be 16-byte aligned");
    PackUpArgs a{weight, (half_t *)fwd, (half_t *)bwd, Cin, Cout};
    LNH_LAUNCH(k_unet_pack_upconv, dim3(div_up((uint64_t)Cin * Cout * 8, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_pack_upconv");
}

int lnh_unet_upconv2x2_backward_data(const void *dy, uint32_t Hd, uint32_t Wd, uint32_t dy_stride, uint32_t dy_offset, uint32_t N,
                                     uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout, const void *weight, void *dx,
                                     lnh_stream_t stream) {
    const char *what = "unet_upconv2x2_backward_data";
    LNH_REQUIRE(dy && weight && dx, LNH_ERR_INVALID_ARG, "%s: null pointer", what);
    UNET_REQUIRE_CHANNELS(what, "Cin", Cin, 64);
    UNET_REQUIRE_CHANNELS(what, "Cout", Cout, 32);
    if (int rc = unet_upconv_dy_window(what, N, H, W, Hd, Wd, dy_stride, dy_offset, Cout)) return rc;
    LNH_REQUIRE(aligned16(dy) && aligned16(weight) && aligned16(dx), LNH_ERR_INVALID_ARG, "%s: every pointer must be 16-byte aligned", what);
    UpBwdArgs a{(const half_t *)dy, (const half_t *)weight, (half_t *)dx, H, W, Hd, Wd, dy_stride, dy_offset, Cin, Cout,
                (uint64_t)N * H * W};
    LNH_LAUNCH(k_unet_upconv_bwd_data, dim3(div_up(a.M, 64), Cin / 64), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_upconv2x2_backward_data");
}

uint64_t lnh_unet_upconv2x2_backward_weight_workspace_size(uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout) {
    if (!upconv_wgrad_shape_ok(N, H, W, Cin, Cout)) return 0;
    const UnetSplit sp = upconv_wgrad_split((uint64_t)N * H * W, Cin, Cout);
    return (uint64_t)sp.S * ((uint64_t)Cin * Cout * 4 + Cout) * sizeof(float);
}

int lnh_unet_upconv2x2_backward_weight(const void *x, const void *dy, uint32_t Hd, uint32_t Wd, uint32_t dy_stride,
                                       uint32_t dy_offset, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout, void *ws,
                                       uint64_t ws_bytes, float *dweight, float *dbias, lnh_stream_t stream) {
    const char *what = "unet_upconv2x2_backward_weight";
    LNH_REQUIRE(x && dy && ws && dweight && dbias, LNH_ERR_INVALID_ARG, "%s: null pointer", what);
    UNET_REQUIRE_CHANNELS(what, "Cin", Cin, 64);
    UNET_REQUIRE_CHANNELS(what, "Cout", Cout, 64);
    if (int rc = unet_upconv_dy_window(what, N, H, W, Hd, Wd, dy_stride, dy_offset, Cout)) return rc;
    const uint64_t need = lnh_unet_upconv2x2_backward_weight_workspace_size(N, H, W, Cin, Cout);
    LNH_REQUIRE(ws_bytes >= need, LNH_ERR_INVALID_ARG, "%s: workspace of %llu bytes, %llu needed", what, (unsigned long long)ws_bytes,
                (unsigned long long)need);
    LNH_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(ws), LNH_ERR_INVALID_ARG, "%s: x, dy and the workspace must be 16-byte aligned",
                what);
    const uint64_t M = (uint64_t)N * H * W, nw = (uint64_t)Cin * Cout * 4, slice = nw + Cout;
    const UnetSplit sp = upconv_wgrad_split(M, Cin, Cout);
    UpWgtArgs a{(const half_t *)x, (const half_t *)dy, (float *)ws, H, W, Hd, Wd, dy_stride, dy_offset, Cin, Cout, M, sp.L};
    const hipStream_t s = (hipStream_t)stream;
    LNH_LAUNCH(k_unet_upconv_bwd_weight, dim3(sp.S, Cin / 64, Cout / 64), dim3(256), 0, s, a);
    LNH_LAUNCH(k_unet_upconv_bwd_reduce, dim3(div_up(slice, 256)), dim3(256), 0, s, (const float *)ws, sp.S, nw, slice, dweight, dbias);
    return lnh_check_launch("lnh_unet_upconv2x2_backward_weight");
}

}  // extern "C"
