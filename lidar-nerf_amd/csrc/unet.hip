// unet.hip — inference of the ray-drop U-Net of the mesh baselines (lidarnvs/unet.py: UNet(10, 1, bilinear=False), eval mode, the
// reference's --amp arithmetic): fp16 NHWC activations, fp16 weights, fp32 accumulation on v_mfma_f32_16x16x32_f16, eval-mode
// BatchNorm + ReLU in fp32 in the epilogue.  Contract: include/lidarnerf_hip.h, lnh_unet_*; DESIGN §18.
//   k_unet_input    [N, C, H, W] f32 -> [N, H, W, 32] fp16, channels C .. 31 zero.
//   k_unet_conv3x3  implicit GEMM, D[co, pixel] = W[co, k] X[k, pixel] with k = (tap, channel): the A operand of an MFMA is 16
//                   output channels x 32 k (8 consecutive fp16 of one weight row per lane), the B operand 32 k x 16 pixels (8
//                   consecutive channels of one NHWC pixel per lane) — both are one 16-byte global read per lane, so nothing is
//                   staged in LDS and no im2col, pooled or concatenated tensor exists: the 2 x 2 maximum is taken over four such
//                   reads, the second source is a second pointer, a tap outside the image (or the second source) is a zero
//                   fragment — the operand rule, written once in unet_common.h (UnetConvGeom) and read there by the weight
//                   gradient too (unet_train_wgrad.hip); this kernel hoists the tap pointers out of its channel loop.  A wave owns MT x 16 pixels (flat over N H W) x 64 output channels; a lane ends with 4 consecutive
//                   channels of one pixel per accumulator: one 8-byte store.  KS: the four waves of a workgroup take the channel
//                   chunks c = w (mod 4) of every tap of ONE 16-pixel tile and add through LDS in a fixed order — the deep levels
//                   (256 pixels, K = 9216) would otherwise fill a quarter of the machine.
//   k_unet_upconv   the same product with k = Cin and rows (2dy + dx, co); every output pixel has one owner.
//   k_unet_head     64 -> 1 per pixel, an fp32 fmaf chain, logits and the mask logit > 0.
// unet_common.h: ld8 / zero8 / max8, aligned16, the pixel bound and decomposition, the sources' geometry check, the channel-range message.
#include "unet_common.h"

namespace {

constexpr uint32_t kLevels = 5;

struct InputArgs {
    const float *in;
    half_t *out;
    uint32_t N, C, H, W;
};

__global__ void __launch_bounds__(256)
k_unet_input(InputArgs a) {
    const uint64_t HW = (uint64_t)a.H * a.W, total = (uint64_t)a.N * HW * 4;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint64_t p = i >> 2;
    const uint32_t grp = (uint32_t)(i & 3);
    const uint64_t n = p / HW, yx = p % HW;
    half8_t v;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t ch = grp * 8 + j;
        v[j] = ch < a.C ? (half_t)a.in[(n * a.C + ch) * HW + yx] : (half_t)0;
    }
    *reinterpret_cast<half8_t *>(a.out + p * 32 + grp * 8) = v;
}

struct ConvArgs {
    UnetConvGeom g;
    const half_t *w;
    const float *scale, *shift;
    half_t *out;
    uint32_t Cout;
    uint64_t M;  // N H W
};

// RAW: the epilogue of the training step, out = fp16(acc) — the convolution in front of batch-statistics BatchNorm and, on the
// flipped and transposed weight image, its data gradient; scale / shift are not read.
template <int MT, bool KS, bool RAW>
__global__ void __launch_bounds__(256)
k_unet_conv3x3(ConvArgs a) {
    static_assert(!KS || MT == 1, "the k-split variant owns one 16-pixel tile");
    __shared__ f32x4 red[KS ? 3 * 4 * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const uint64_t base = KS ? (uint64_t)blockIdx.x * 16 : ((uint64_t)blockIdx.x * 4 + wave) * (16 * MT);
    if (!KS && base >= a.M) return;  // (no barrier in this variant)
    const UnetConvGeom &G = a.g;
    const uint32_t co0 = blockIdx.y * 64, Ct = G.C0 + G.C1;
    bool valid[MT];
    uint32_t pn[MT];
    int py[MT], px[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const uint64_t p = base + m * 16 + c;
        valid[m] = p < a.M;
        const UnetPixel q = unet_pixel(valid[m] ? p : 0, G.H, G.W);
        pn[m] = q.n, py[m] = (int)q.y, px[m] = (int)q.x;
    }
    const half_t *wrow[4];
#pragma unroll
    for (int t = 0; t < 4; t++) wrow[t] = a.w + (uint64_t)(co0 + 16 * t + c) * 9 * Ct + 8 * g;
    f32x4 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[m][t] = f32x4{0, 0, 0, 0};
    const uint32_t ch_first = KS ? wave * 32 : 0, ch_step = KS ? 128 : 32;

    for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        bool in0[MT], in1[MT];
        const half_t *p0[MT], *p1[MT];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            const int yy = py[m] + dy, xx = px[m] + dx;
            in0[m] = unet_tap_in0(G, valid[m], yy, xx);
            in1[m] = unet_tap_in1(G, in0[m], yy, xx);
            p0[m] = in0[m] ? unet_tap_src0(G, pn[m], yy, xx) + 8 * g : G.s0;
            p1[m] = in1[m] ? unet_tap_src1(G, pn[m], yy, xx) + 8 * g : G.s0;
        }
        const uint32_t k0 = tap * Ct;
#pragma unroll 2
        for (uint32_t ch = ch_first; ch < G.C0; ch += ch_step) {
            half8_t wf[4], xf[MT];
#pragma unroll
            for (int t = 0; t < 4; t++) wf[t] = ld8(wrow[t] + k0 + ch);
#pragma unroll
            for (int m = 0; m < MT; m++) xf[m] = in0[m] ? unet_ld8_src0(G, p0[m] + ch) : zero8();
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int t = 0; t < 4; t++) acc[m][t] = UNET_MFMA(wf[t], xf[m], acc[m][t]);
        }
        // the second source continues the chunk count of the first, so the k-split stays balanced when C0 / 32 is no multiple of 4
        const uint32_t first1 = KS ? ((wave + 4 - (G.C0 / 32) % 4) % 4) * 32 : 0;
#pragma unroll 2
        for (uint32_t ch = first1; ch < G.C1; ch += ch_step) {
            half8_t wf[4], xf[MT];
#pragma unroll
            for (int t = 0; t < 4; t++) wf[t] = ld8(wrow[t] + k0 + G.C0 + ch);
#pragma unroll
            for (int m = 0; m < MT; m++) xf[m] = in1[m] ? ld8(p1[m] + ch) : zero8();
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int t = 0; t < 4; t++) acc[m][t] = UNET_MFMA(wf[t], xf[m], acc[m][t]);
        }
    }
    if constexpr (KS) {
        if (wave > 0) {
#pragma unroll
            for (int t = 0; t < 4; t++) red[((wave - 1) * 4 + t) * 64 + lane] = acc[0][t];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int t = 0; t < 4; t++)
            acc[0][t] = (acc[0][t] + red[(0 * 4 + t) * 64 + lane]) + (red[(1 * 4 + t) * 64 + lane] + red[(2 * 4 + t) * 64 + lane]);
    }
#pragma unroll
    for (int m = 0; m < MT; m++) {
        if (!valid[m]) continue;
        const uint64_t p = base + m * 16 + c;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t co = co0 + 16 * t + 4 * g;
            half4_t o;
            if constexpr (RAW) {
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = (half_t)acc[m][t][r];
            } else {
                const f32x4 s = *reinterpret_cast<const f32x4 *>(a.scale + co), sh = *reinterpret_cast<const f32x4 *>(a.shift + co);
#pragma unroll
                for (int r = 0; r < 4; r++) o[r] = (half_t)fmaxf(fmaf(acc[m][t][r], s[r], sh[r]), 0.0f);
            }
            *reinterpret_cast<half4_t *>(a.out + p * a.Cout + co) = o;
        }
    }
}

struct UpArgs {
    const half_t *in, *w;
    const float *bias;
    half_t *out;
    uint32_t H, W, Cin, Cout;
    uint64_t M;  // N H W of the input
};

__global__ void __launch_bounds__(256)
k_unet_upconv(UpArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const uint64_t base = ((uint64_t)blockIdx.x * 4 + wave) * 16;
    if (base >= a.M) return;
    const uint32_t j0 = blockIdx.y * 64;  // row (2dy + dx) * Cout + co of the [4 Cout, Cin] matrix; Cout is a multiple of 64
    const uint32_t q = j0 / a.Cout, co0 = j0 % a.Cout;
    const uint64_t p = base + c;
    const bool valid = p < a.M;
    const half_t *x = a.in + (valid ? p : 0) * a.Cin + 8 * g;
    const half_t *wrow[4];
#pragma unroll
    for (int t = 0; t < 4; t++) wrow[t] = a.w + (uint64_t)(j0 + 16 * t + c) * a.Cin + 8 * g;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{0, 0, 0, 0};
#pragma unroll 4
    for (uint32_t ch = 0; ch < a.Cin; ch += 32) {
        half8_t wf[4];
#pragma unroll
        for (int t = 0; t < 4; t++) wf[t] = ld8(wrow[t] + ch);
        const half8_t xf = valid ? ld8(x + ch) : zero8();
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = UNET_MFMA(wf[t], xf, acc[t]);
    }
    if (!valid) return;
    const UnetPixel px = unet_pixel(p, a.H, a.W);
    const uint64_t op = ((uint64_t)px.n * (2 * a.H) + (2 * px.y + (q >> 1))) * (2 * (uint64_t)a.W) + (2 * px.x + (q & 1));
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t co = co0 + 16 * t + 4 * g;
        const f32x4 b = *reinterpret_cast<const f32x4 *>(a.bias + co);
        half4_t o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = (half_t)(acc[t][r] + b[r]);
        *reinterpret_cast<half4_t *>(a.out + op * a.Cout + co) = o;
    }
}

struct HeadArgs {
    const half_t *in, *w;
    const float *bias;
    float *logits, *mask;
    uint64_t M;
};

__global__ void __launch_bounds__(256)
k_unet_head(HeadArgs a) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.M) return;
    float o = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const half8_t x = ld8(a.in + p * 64 + 8 * k), w = ld8(a.w + 8 * k);
#pragma unroll
        for (int j = 0; j < 8; j++) o = fmaf((float)x[j], (float)w[j], o);
    }
    o += a.bias[0];
    a.logits[p] = o;
    if (a.mask) a.mask[p] = o > 0.0f ? 1.0f : 0.0f;  // false for NaN
}

uint64_t pad256(uint64_t b) { return (b + 255) / 256 * 256; }

// lnh_unet_conv3x3 and lnh_unet_conv3x3_raw: one set of checks, one tile rule, one main loop; RAW picks the epilogue.
template <bool RAW>
int conv3x3_launch(const char *what, const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool, const void *src1,
                   uint32_t C1, uint32_t H1, uint32_t W1, const void *weight, const float *scale, const float *shift, uint32_t N,
                   uint32_t Cout, uint32_t tile, void *out, lnh_stream_t stream) {
    LNH_REQUIRE(src0 && weight && (RAW || (scale && shift)) && out, LNH_ERR_INVALID_ARG, "%s: null pointer", what);
    LNH_REQUIRE(pool <= 1, LNH_ERR_INVALID_ARG, "%s: pool %u (0 or 1)", what, pool);
    UNET_REQUIRE_CHANNELS(what, "C0", C0, 32);
    LNH_REQUIRE(C1 <= 1024 && C1 % 32 == 0, LNH_ERR_INVALID_ARG, "%s: C1 %u (a multiple of 32 up to 1024)", what, C1);
    LNH_REQUIRE((C1 != 0) == (src1 != nullptr), LNH_ERR_INVALID_ARG, "%s: src1 and C1 must be given together", what);
    UNET_REQUIRE_CHANNELS(what, "Cout", Cout, 64);
    ConvArgs a{};
    a.g = UnetConvGeom{(const half_t *)src0, (const half_t *)src1, 0, 0, H0, W0, C0, H1, W1, C1, pool};
    if (int rc = unet_conv_geometry(what, N, a.g)) return rc;
    LNH_REQUIRE(aligned16(src0) && aligned16(src1) && aligned16(weight) && aligned16(scale) && aligned16(shift) && aligned16(out),
                LNH_ERR_INVALID_ARG, "%s: every pointer must be 16-byte aligned", what);
    LNH_REQUIRE(tile == 0 || tile == LNH_UNET_TILE_16 || tile == LNH_UNET_TILE_32 || tile == LNH_UNET_TILE_64 ||
                    tile == LNH_UNET_TILE_KSPLIT,
                LNH_ERR_INVALID_ARG, "%s: tile %u (0, 1, 2, 4 or 8)", what, tile);
    a.w = (const half_t *)weight; a.scale = scale; a.shift = shift; a.out = (half_t *)out;
    a.Cout = Cout;
    a.M = (uint64_t)N * a.g.H * a.g.W;
    const uint32_t cols = Cout / 64;
    if (tile == 0) {
        // From the timings of every layer of a 66 x 1030 frame with every tile: the operand reads are hidden by waves
        // in flight, so a large tile pays only where it leaves two waves per SIMD (2048), or one wave per two SIMDs with a long k
        // loop; everything smaller — 17 k pixels and fewer — runs fastest with the k range split over a workgroup's waves.
        auto waves = [&](uint32_t mt) { return (a.M + 16 * mt - 1) / (16 * mt) * cols; };
        const uint32_t K = 9 * (C0 + C1);
        if (waves(2) >= 2048) tile = K >= 1024 ? LNH_UNET_TILE_64 : LNH_UNET_TILE_32;
        else if (waves(4) >= 512 && K >= 2048) tile = LNH_UNET_TILE_64;
        else tile = LNH_UNET_TILE_KSPLIT;
    }
    const hipStream_t s = (hipStream_t)stream;
    if (tile == LNH_UNET_TILE_KSPLIT) LNH_LAUNCH((k_unet_conv3x3<1, true, RAW>), dim3(div_up(a.M, 16), cols), dim3(256), 0, s, a);
    else if (tile == LNH_UNET_TILE_16) LNH_LAUNCH((k_unet_conv3x3<1, false, RAW>), dim3(div_up(a.M, 64), cols), dim3(256), 0, s, a);
    else if (tile == LNH_UNET_TILE_32) LNH_LAUNCH((k_unet_conv3x3<2, false, RAW>), dim3(div_up(a.M, 128), cols), dim3(256), 0, s, a);
    else LNH_LAUNCH((k_unet_conv3x3<4, false, RAW>), dim3(div_up(a.M, 256), cols), dim3(256), 0, s, a);
    return lnh_check_launch(RAW ? "lnh_unet_conv3x3_raw" : "lnh_unet_conv3x3");
}

}  // namespace

extern "C" {

uint64_t lnh_unet_workspace_size(uint32_t N, uint32_t H, uint32_t W) {
    if (N == 0 || H < 16 || W < 16 || (uint64_t)N * H * W > kUnetMaxPixels) return 0;
    uint64_t total = pad256((uint64_t)N * H * W * 32 * 2);
    for (uint32_t l = 0; l < kLevels; l++)  // DoubleConv: mid and output of every encoder level
        total += 2 * pad256((uint64_t)N * (H >> l) * (W >> l) * (64u << l) * 2);
    for (uint32_t l = 0; l + 1 < kLevels; l++)  // decoder: the transposed convolution's output and the block's output
        total += pad256((uint64_t)N * (2 * (H >> (l + 1))) * (2 * (W >> (l + 1))) * (64u << l) * 2) +
                 pad256((uint64_t)N * (H >> l) * (W >> l) * (64u << l) * 2);
    return total;
}

int lnh_unet_input(const float *in, uint32_t N, uint32_t C, uint32_t H, uint32_t W, void *out, lnh_stream_t stream) {
    LNH_REQUIRE(in && out, LNH_ERR_INVALID_ARG, "unet_input: null pointer");
    LNH_REQUIRE(C >= 1 && C <= 32, LNH_ERR_INVALID_ARG, "unet_input: %u channels (1 .. 32)", C);
    LNH_REQUIRE(N && H && W && (uint64_t)N * H * W <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "unet_input: image [%u, %u, %u] (1 .. 2^26 pixels)", N, H, W);
    LNH_REQUIRE(aligned16(out), LNH_ERR_INVALID_ARG, "unet_input: out must be 16-byte aligned");
    InputArgs a{in, (half_t *)out, N, C, H, W};
    LNH_LAUNCH(k_unet_input, dim3(div_up((uint64_t)N * H * W * 4, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_input");
}

int lnh_unet_conv3x3(const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool, const void *src1, uint32_t C1,
                     uint32_t H1, uint32_t W1, const void *weight, const float *scale, const float *shift, uint32_t N,
                     uint32_t Cout, uint32_t tile, void *out, lnh_stream_t stream) {
    return conv3x3_launch<false>("unet_conv3x3", src0, C0, H0, W0, pool, src1, C1, H1, W1, weight, scale, shift, N, Cout, tile, out,
                                 stream);
}

int lnh_unet_conv3x3_raw(const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool, const void *src1, uint32_t C1,
                         uint32_t H1, uint32_t W1, const void *weight, uint32_t N, uint32_t Cout, uint32_t tile, void *out,
                         lnh_stream_t stream) {
    return conv3x3_launch<true>("unet_conv3x3_raw", src0, C0, H0, W0, pool, src1, C1, H1, W1, weight, nullptr, nullptr, N, Cout, tile,
                                out, stream);
}

int lnh_unet_upconv2x2(const void *in, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, const void *weight, const float *bias,
                       uint32_t Cout, void *out, lnh_stream_t stream) {
    LNH_REQUIRE(in && weight && bias && out, LNH_ERR_INVALID_ARG, "unet_upconv2x2: null pointer");
    UNET_REQUIRE_CHANNELS("unet_upconv2x2", "Cin", Cin, 32);
    UNET_REQUIRE_CHANNELS("unet_upconv2x2", "Cout", Cout, 64);
    LNH_REQUIRE(N && H && W && (uint64_t)N * H * W * 4 <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "unet_upconv2x2: image [%u, %u, %u] (output of 1 .. 2^26 pixels)", N, H, W);
    LNH_REQUIRE(aligned16(in) && aligned16(weight) && aligned16(bias) && aligned16(out), LNH_ERR_INVALID_ARG,
                "unet_upconv2x2: every pointer must be 16-byte aligned");
    UpArgs a{(const half_t *)in, (const half_t *)weight, bias, (half_t *)out, H, W, Cin, Cout, (uint64_t)N * H * W};
    LNH_LAUNCH(k_unet_upconv, dim3(div_up(a.M, 64), 4 * Cout / 64), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_upconv2x2");
}

int lnh_unet_head(const void *in, uint32_t N, uint32_t H, uint32_t W, const void *weight, const float *bias, float *logits,
                  float *mask, lnh_stream_t stream) {
    LNH_REQUIRE(in && weight && bias && logits, LNH_ERR_INVALID_ARG, "unet_head: null pointer");
    LNH_REQUIRE(N && H && W && (uint64_t)N * H * W <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "unet_head: image [%u, %u, %u] (1 .. 2^26 pixels)", N, H, W);
    LNH_REQUIRE(aligned16(in) && aligned16(weight), LNH_ERR_INVALID_ARG, "unet_head: in and weight must be 16-byte aligned");
    HeadArgs a{(const half_t *)in, (const half_t *)weight, bias, logits, mask, (uint64_t)N * H * W};
    LNH_LAUNCH(k_unet_head, dim3(div_up(a.M, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_unet_head");
}

}  // extern "C"
