// unet_train_wgrad.hip — the weight gradient of the ray-drop U-Net's 3 x 3 convolutions.  Contract:
// include/lidarnerf_hip.h, "U-Net training", lnh_unet_conv3x3_backward_weight.
//   dW[co, ci, t] = sum over the M = N H W output pixels p of dz[p, co] X[p + off(t), ci], t = 3 (dy + 1) + (dx + 1) the FORWARD tap.
//   X is the operand k_unet_conv3x3 (csrc/unet.hip) read and exists nowhere: source 0, max-pooled 2 x 2 on read (floor), then the
//   channels of source 1, which reads as zero for y >= H1 or x >= W1; a tap outside the image is zero.  The rule is unet_common.h's
//   (UnetConvGeom and its functions: which source, which address, the maximum's chain of comparisons), called by both kernels; the
//   sources' geometry check and the slice split (unet_pixel_split) are there too.  fp16 operands, fp32 sums on v_mfma_f32_16x16x32_f16, no float atomics.
//   k_unet_conv_wgrad   the summed index (the pixel) is the slow memory index of both operands, so workgroup (slice, ci block, co
//                       block) walks its pixel slice in steps of 32: thread (pixel r = t / 8, chunk t % 8) reads 8 channels of dz and,
//                       for each of the nine taps, 8 channels of X at the shifted pixel (16-byte reads, four and a maximum where
//                       pooled; a pixel past the slice, a tap outside the image, a channel past C0 + C1 are zero, never branched
//                       around the LDS traffic) into registers one step ahead, and stores them as rows of [pixel][80 halves] LDS
//                       tiles: one of dz, nine of X.  Wave w owns the ci 16 w .. 16 w + 15 of the block, all 64 co and the nine taps:
//                       36 accumulators (144 registers) fed per step by 9 X fragments and 4 dz fragments — the dz tile is shared by
//                       the taps and every fragment is read once per wave.  MFMA k = 8 g + 4 h + q (g = lane / 16) is tile row
//                       16 (g / 2) + 8 h + 4 (g % 2) + q in both operands.
//                       TR:  a fragment is two ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group addresses row q, columns 4 p ..
//                            4 p + 3 of a 4 x 16 block and receives column (lane % 16), rows 0 .. 3.  All 256 threads take every
//                            read (EXEC all ones: tiles are padded, not masked), addresses are multiples of 8 bytes.  Banks, by the
//                            rule bank = (byte / 4) % 64 per 32-lane half: a half reads 8 consecutive tile rows x 32 bytes, row
//                            pitch 160 bytes = 40 dwords, and r 40 mod 64 for r = 0 .. 7 is {0, 40, 16, 56, 32, 8, 48, 24}: eight
//                            distinct 8-dword slots, conflict-free.  (With the upconv kernel's row order 4 j + g a half would read
//                            rows r and r + 8, 320 dwords = 0 mod 64 apart: 2-way; hence the row order above.)
//                       !TR: the same fragments gathered with sixteen 16-bit LDS reads each; same k order, same bits.
//                       The partial sums go to the workspace as [slice][tap][co][Cp] f32 (Cp = C0 + C1), 16-byte stores.
//   k_unet_conv_wgrad_finish   thread (co, ci < Cin) adds the slices of its nine taps in ascending order in float64, rounds once
//                       and writes nine consecutive floats of the parameter's [Cout, Cin, 3, 3] layout: the transposition happens
//                       here, and channels Cin .. Cp - 1 of the padded first layer are never written.  With more than 8 slices
//                       k_unet_conv_wgrad_finish_wide does the same with one thread per element (same order, same bits).
//   The split, from the shape alone: S = min(ceil(M / 256), max(1, floor(32 MiB / (36 Cp Cout)))) slices of L = ceil(M / S) rounded
//   up to the 32-pixel step, then S = ceil(M / L): 266 slices for the first layer of a 66 x 1030 frame, one for every layer of
//   256 x 512 channels and more (the deepest: one 37.7 MB partial).  Same shape, same bits.
#include "unet_common.h"

namespace {

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));  // what the transposed-read builtin returns

constexpr uint32_t kWgPitch = 80;                 // halves per LDS row of 64 channels (160 bytes: see the bank picture above)
constexpr uint64_t kWgSliceBudget = 32ull << 20;  // bytes of partials the split rule allows itself

struct WgradArgs {
    UnetConvGeom g;
    const half_t *dz;
    float *part;  // [S][9][Cout][Cp]
    uint32_t Cout;
    uint64_t M, L;  // output pixels; pixels per slice (a multiple of 32)
};

template <bool TR>
__device__ __forceinline__ half8_t fragment(const half_t *tile, uint32_t col, uint32_t lane) {
    const uint32_t g = lane >> 4, row0 = 16 * (g >> 1) + 4 * (g & 1);
    half8_t f;
    if constexpr (TR) {
        const uint32_t q = (lane & 15) >> 2, p = lane & 3;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const half_t *src = tile + (row0 + 8 * h + q) * kWgPitch + col + 4 * p;
            const half4_t v = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                                                              (__attribute__((address_space(3))) fp16x4_t *)src));
#pragma unroll
            for (int j = 0; j < 4; j++) f[4 * h + j] = v[j];
        }
    } else {
        const uint32_t c = lane & 15;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int j = 0; j < 4; j++) f[4 * h + j] = tile[(row0 + 8 * h + j) * kWgPitch + col + c];
    }
    return f;
}

template <bool TR>
__global__ void __launch_bounds__(256)
k_unet_conv_wgrad(WgradArgs a) {
    __shared__ __attribute__((aligned(16))) half_t xs[9][32 * kWgPitch];
    __shared__ __attribute__((aligned(16))) half_t ds[32 * kWgPitch];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, c = lane & 15, g = lane >> 4;
    const uint32_t spix = t >> 3, chunk = t & 7;  // this thread's tile row and 8-channel chunk when staging
    const UnetConvGeom &G = a.g;
    const uint32_t ci0 = blockIdx.y * 64, co0 = blockIdx.z * 64, Cp = G.C0 + G.C1;
    const uint64_t begin = (uint64_t)blockIdx.x * a.L, end = begin + a.L < a.M ? begin + a.L : a.M;
    const uint32_t ch = ci0 + 8 * chunk;                // the staged channels ch .. ch + 7 of the concatenated operand:
    const int kind = ch < G.C0 ? 0 : ch < Cp ? 1 : 2;  // source 0, source 1, or past the last channel (zero)

    half8_t xr[9], dr;
    auto fetch = [&](uint64_t base) {
        const uint64_t p = base + spix;
        const bool valid = p < end;
        const UnetPixel q = unet_pixel(valid ? p : 0, G.H, G.W);
        dr = valid ? ld8(a.dz + p * a.Cout + co0 + 8 * chunk) : zero8();
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int yy = (int)q.y + tap / 3 - 1, xx = (int)q.x + tap % 3 - 1;
            const bool in0 = unet_tap_in0(G, valid, yy, xx);
            half8_t v = zero8();
            if (kind == 0 && in0) v = unet_ld8_src0(G, unet_tap_src0(G, q.n, yy, xx) + ch);
            else if (kind == 1 && unet_tap_in1(G, in0, yy, xx)) v = ld8(unet_tap_src1(G, q.n, yy, xx) + (ch - G.C0));
            xr[tap] = v;
        }
    };

    f32x4 acc[9][4];
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[tap][j] = f32x4{0, 0, 0, 0};

    fetch(begin);
    for (uint64_t base = begin; base < end; base += 32) {  // (a trip count of the workgroup: every thread takes every LDS read)
        *reinterpret_cast<half8_t *>(&ds[spix * kWgPitch + 8 * chunk]) = dr;
#pragma unroll
        for (int tap = 0; tap < 9; tap++) *reinterpret_cast<half8_t *>(&xs[tap][spix * kWgPitch + 8 * chunk]) = xr[tap];
        __syncthreads();
        if (base + 32 < end) fetch(base + 32);  // the next step's reads fly over this step's products
        half8_t bf[4];
#pragma unroll
        for (int j = 0; j < 4; j++) bf[j] = fragment<TR>(ds, 16 * j, lane);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const half8_t af = fragment<TR>(xs[tap], 16 * wave, lane);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[tap][j] = UNET_MFMA(af, bf[j], acc[tap][j]);
        }
        __syncthreads();
    }
    const uint32_t ci = ci0 + 16 * wave + 4 * g;  // accumulator element r is row 4 g + r of the A operand: ci + r
    if (ci >= Cp) return;                         // (the padded half of the first layer's 64-channel block)
    float *dst = a.part + (uint64_t)blockIdx.x * 9 * a.Cout * Cp;
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            *reinterpret_cast<f32x4 *>(dst + ((uint64_t)tap * a.Cout + co0 + 16 * j + c) * Cp + ci) = acc[tap][j];
}

// Both finishing kernels add the slices of an element in ascending order in float64 and round once; they differ in who owns what.
// Few slices (S <= kWgFinishWide), large gradients: thread (co, ci) owns its nine taps and writes 36 consecutive bytes.
__global__ void __launch_bounds__(256)
k_unet_conv_wgrad_finish(const float *__restrict__ part, uint32_t S, uint32_t Cout, uint32_t Cp, uint32_t Cin,
                         float *__restrict__ dweight) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)Cout * Cin) return;
    const uint32_t co = (uint32_t)(i / Cin), ci = (uint32_t)(i % Cin);
    const uint64_t plane = (uint64_t)Cout * Cp, slice = 9 * plane;
    const float *src = part + (uint64_t)co * Cp + ci;
    double s[9];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) s[tap] = 0.0;
    for (uint32_t k = 0; k < S; k++) {  // (nine independent reads per slice: S memory latencies, not 9 S)
#pragma unroll
        for (int tap = 0; tap < 9; tap++) s[tap] += (double)src[(uint64_t)k * slice + tap * plane];
    }
#pragma unroll
    for (int tap = 0; tap < 9; tap++) dweight[i * 9 + tap] = (float)s[tap];
}

// Many slices, small gradients (a slice of partials is then at most 32 MiB / 9): thread (tap, co, ci) owns one element, reads eight
// slices at a time and adds them in order — one thread per (co, ci) chained 9 S memory latencies, most of the top level's time.
constexpr uint32_t kWgFinishWide = 8;

__global__ void __launch_bounds__(256)
k_unet_conv_wgrad_finish_wide(const float *__restrict__ part, uint32_t S, uint32_t Cout, uint32_t Cp, uint32_t Cin,
                              float *__restrict__ dweight) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, n = (uint64_t)Cout * Cin;
    if (i >= 9 * n) return;
    const uint32_t tap = (uint32_t)(i / n), co = (uint32_t)(i % n / Cin), ci = (uint32_t)(i % Cin);
    const uint64_t plane = (uint64_t)Cout * Cp, slice = 9 * plane;
    const float *src = part + tap * plane + (uint64_t)co * Cp + ci;
    double s = 0.0;
    uint32_t k = 0;
    for (; k + 8 <= S; k += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = src[(uint64_t)(k + j) * slice];
#pragma unroll
        for (int j = 0; j < 8; j++) s += (double)v[j];
    }
    for (; k < S; k++) s += (double)src[(uint64_t)k * slice];
    dweight[(i % n) * 9 + tap] = (float)s;
}

UnetSplit conv_wgrad_split(uint64_t M, uint32_t Cp, uint32_t Cout) { return unet_pixel_split(M, 36ull * Cp * Cout, kWgSliceBudget); }

bool conv_wgrad_shape_ok(uint32_t N, uint32_t H0, uint32_t W0, uint32_t pool, uint32_t C0, uint32_t C1, uint32_t Cout) {
    if (pool > 1 || !N || !H0 || !W0 || (uint64_t)N * H0 * W0 > kUnetMaxPixels) return false;
    if (!(pool ? H0 / 2 : H0) || !(pool ? W0 / 2 : W0)) return false;
    const bool c0_ok = C0 == 32 ? C1 == 0 : (unet_channels_ok(C0, 64) && (C1 == 0 || C1 == C0));
    return c0_ok && unet_channels_ok(Cout, 64);
}

}  // namespace

extern "C" {

uint64_t lnh_unet_conv3x3_backward_weight_workspace_size(uint32_t N, uint32_t H0, uint32_t W0, uint32_t pool, uint32_t C0,
                                                         uint32_t C1, uint32_t Cout) {
    if (!conv_wgrad_shape_ok(N, H0, W0, pool, C0, C1, Cout)) return 0;
    const uint64_t M = (uint64_t)N * (pool ? H0 / 2 : H0) * (pool ? W0 / 2 : W0);
    return (uint64_t)conv_wgrad_split(M, C0 + C1, Cout).S * 9 * Cout * (C0 + C1) * sizeof(float);
}

int lnh_unet_conv3x3_backward_weight(const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool, const void *src1,
                                     uint32_t C1, uint32_t H1, uint32_t W1, const void *dz, uint32_t N, uint32_t Cout, uint32_t Cin,
                                     uint32_t variant, void *ws, uint64_t ws_bytes, float *dweight, lnh_stream_t stream) {
    const char *what = "unet_conv3x3_backward_weight";
    LNH_REQUIRE(src0 && dz && ws && dweight, LNH_ERR_INVALID_ARG, "%s: null pointer", what);
    LNH_REQUIRE(pool <= 1, LNH_ERR_INVALID_ARG, "%s: pool %u (0 or 1)", what, pool);
    LNH_REQUIRE(C0 == 32 || unet_channels_ok(C0, 64), LNH_ERR_INVALID_ARG,
                "%s: C0 %u (32, or a multiple of 64 up to 1024)", what, C0);
    LNH_REQUIRE(C1 == 0 || (C1 == C0 && C0 != 32), LNH_ERR_INVALID_ARG, "%s: C1 %u beside C0 %u (0, or C0 where C0 is a multiple of 64)",
                what, C1, C0);
    LNH_REQUIRE((C1 != 0) == (src1 != nullptr), LNH_ERR_INVALID_ARG, "%s: src1 and C1 must be given together", what);
    UNET_REQUIRE_CHANNELS(what, "Cout", Cout, 64);
    LNH_REQUIRE(C0 == 32 ? (Cin >= 1 && Cin <= 32) : Cin == C0 + C1, LNH_ERR_INVALID_ARG,
                "%s: Cin %u (C0 + C1 = %u; 1 .. 32 for the padded first layer, C0 = 32)", what, Cin, C0 + C1);
    WgradArgs a{};
    a.g = UnetConvGeom{(const half_t *)src0, (const half_t *)src1, 0, 0, H0, W0, C0, H1, W1, C1, pool};
    if (int rc = unet_conv_geometry(what, N, a.g)) return rc;
    LNH_REQUIRE(variant <= LNH_UNET_WGRAD_TR, LNH_ERR_INVALID_ARG, "%s: variant %u (0, 1 or 2)", what, variant);
    const uint64_t need = lnh_unet_conv3x3_backward_weight_workspace_size(N, H0, W0, pool, C0, C1, Cout);
    LNH_REQUIRE(need && ws_bytes >= need, LNH_ERR_INVALID_ARG, "%s: workspace of %llu bytes, %llu needed", what,
                (unsigned long long)ws_bytes, (unsigned long long)need);
    LNH_REQUIRE(aligned16(src0) && aligned16(src1) && aligned16(dz) && aligned16(ws) && aligned16(dweight), LNH_ERR_INVALID_ARG,
                "%s: every pointer must be 16-byte aligned", what);
    const uint32_t Cp = C0 + C1;
    a.dz = (const half_t *)dz; a.part = (float *)ws; a.Cout = Cout;
    a.M = (uint64_t)N * a.g.H * a.g.W;
    const UnetSplit sp = conv_wgrad_split(a.M, Cp, Cout);
    a.L = sp.L;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(sp.S, (Cp + 63) / 64, Cout / 64);
    if (variant == LNH_UNET_WGRAD_GATHER) LNH_LAUNCH((k_unet_conv_wgrad<false>), grid, dim3(256), 0, s, a);
    else LNH_LAUNCH((k_unet_conv_wgrad<true>), grid, dim3(256), 0, s, a);
    if (sp.S <= kWgFinishWide)
        LNH_LAUNCH(k_unet_conv_wgrad_finish, dim3(div_up((uint64_t)Cout * Cin, 256)), dim3(256), 0, s, (const float *)ws, sp.S, Cout, Cp,
                   Cin, dweight);
    else
        LNH_LAUNCH(k_unet_conv_wgrad_finish_wide, dim3(div_up(9ull * Cout * Cin, 256)), dim3(256), 0, s, (const float *)ws, sp.S, Cout,
                   Cp, Cin, dweight);
    return lnh_check_launch("lnh_unet_conv3x3_backward_weight");
}

}  // extern "C"
