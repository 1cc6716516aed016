// unet_common.h — what the five unet*.hip files of the ray-drop U-Net share: the small vector helpers, the operand
// rule of the 3 x 3 convolution (read by k_unet_conv3x3 in unet.hip and by k_unet_conv_wgrad in unet_train_wgrad.hip: the weight
// gradient is correct only while both read the same operand, so there is one copy), and the host checks more than one entry point
// makes.  Each entry point keeps the checks only it has and its own order of refusal (tests/golden/unet_host.json pins it).
#pragma once
#include "common.h"

typedef float4_t f32x4;
#define UNET_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)

constexpr uint64_t kUnetMaxPixels = 1ull << 26;

__host__ __device__ inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ half8_t ld8(const half_t *p) { return *reinterpret_cast<const half8_t *>(p); }
__device__ __forceinline__ half8_t zero8() { return half8_t{0, 0, 0, 0, 0, 0, 0, 0}; }
// The 2 x 2 maximum is max8(max8(a, b), max8(c, d)) of these comparisons wherever a pooled operand is formed: a > b ? a : b keeps b
// for a NaN in either place and for -0 against +0, so another chain (or fmax) would give the forward and the weight gradient
// operands that differ in such elements.
__device__ __forceinline__ half8_t max8(half8_t a, half8_t b) {
    half8_t r;
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = a[i] > b[i] ? a[i] : b[i];
    return r;
}

// flat pixel p of an [N, H, W] image (p < 2^26 pixels)
struct UnetPixel {
    uint32_t n, y, x;
};
__device__ __forceinline__ UnetPixel unet_pixel(uint64_t p, uint32_t H, uint32_t W) {
    const uint64_t HW = (uint64_t)H * W;
    const uint32_t yx = (uint32_t)(p % HW);
    return UnetPixel{(uint32_t)(p / HW), yx / W, yx % W};
}

// ---- the operand of the 3 x 3 convolution ------------------------------------------------------------------------------------------------
// X[pixel, tap, channel] exists nowhere.  Channels [0, C0) are source 0 [N, H0, W0, C0], max-pooled 2 x 2 on read where pool (floor:
// H = H0 / 2), channels [C0, C0 + C1) source 1 [N, H1, W1, C1], which is the output's size or one row / column smaller and reads as
// zero there; a tap outside the H x W image is zero.
struct UnetConvGeom {
    const half_t *s0, *s1;
    uint32_t H, W, H0, W0, C0, H1, W1, C1, pool;
};

// tap (yy, xx) of a valid pixel lies in source 0 / of a tap in source 0: in source 1 as well
__device__ __forceinline__ bool unet_tap_in0(const UnetConvGeom &g, bool valid, int yy, int xx) {
    return valid && yy >= 0 && yy < (int)g.H && xx >= 0 && xx < (int)g.W;
}
__device__ __forceinline__ bool unet_tap_in1(const UnetConvGeom &g, bool in0, int yy, int xx) {
    return in0 && g.C1 != 0 && yy < (int)g.H1 && xx < (int)g.W1;
}
// channel 0 of such a tap: in source 0 (the upper left pixel of its window where pooled) and in source 1
__device__ __forceinline__ const half_t *unet_tap_src0(const UnetConvGeom &g, uint32_t n, int yy, int xx) {
    const uint32_t sy = g.pool ? 2 * yy : yy, sx = g.pool ? 2 * xx : xx;  // (2 yy + 1 <= 2 H - 1 <= H0 - 1)
    return g.s0 + (((uint64_t)n * g.H0 + sy) * g.W0 + sx) * g.C0;
}
__device__ __forceinline__ const half_t *unet_tap_src1(const UnetConvGeom &g, uint32_t n, int yy, int xx) {
    return g.s1 + (((uint64_t)n * g.H1 + yy) * g.W1 + xx) * g.C1;
}
// eight channels of source 0 at p = unet_tap_src0(..) + channel, pooled on read
__device__ __forceinline__ half8_t unet_ld8_src0(const UnetConvGeom &g, const half_t *p) {
    half8_t v = ld8(p);
    if (g.pool) {
        const uint64_t row = (uint64_t)g.W0 * g.C0;  // one source-0 row, in elements
        v = max8(v, ld8(p + g.C0));
        v = max8(v, max8(ld8(p + row), ld8(p + row + g.C0)));
    }
    return v;
}

// ---- host checks --------------------------------------------------------------------------------------------------------------------------
static inline bool unet_channels_ok(uint32_t C, uint32_t step) { return C >= step && C <= 1024 && C % step == 0; }
// `what` is the entry point's name without lnh_, `name` the argument's
#define UNET_REQUIRE_CHANNELS(what, name, C, step)                                                                                 \
    LNH_REQUIRE(unet_channels_ok((C), (step)), LNH_ERR_INVALID_ARG, "%s: %s %u (a multiple of %u, %u .. 1024)", (what), (name), (C), \
                (uint32_t)(step), (uint32_t)(step))

// What lnh_unet_conv3x3, _raw and _backward_weight require of the sources' sizes alike; fills the output size g.H, g.W.
static inline int unet_conv_geometry(const char *what, uint32_t N, UnetConvGeom &g) {
    g.H = g.pool ? g.H0 / 2 : g.H0;
    g.W = g.pool ? g.W0 / 2 : g.W0;
    LNH_REQUIRE(N && g.H && g.W && (uint64_t)N * g.H0 * g.W0 <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "%s: source [%u, %u, %u], pool %u (output of 1 .. 2^26 pixels)", what, N, g.H0, g.W0, g.pool);
    if (g.C1) {
        LNH_REQUIRE(g.H1 <= g.H && g.H - g.H1 <= 1 && g.W1 <= g.W && g.W - g.W1 <= 1 && g.H1 && g.W1, LNH_ERR_INVALID_ARG,
                    "%s: second source %u x %u under an output of %u x %u (each 0 or 1 smaller)", what, g.H1, g.W1, g.H, g.W);
    }
    return LNH_OK;
}

// What both backward entry points of the transposed convolution require of the image and of dy, the gradient of its [N, 2H, 2W, Cout]
// output read in place: channels [off, off + Cout) of a tensor [N, Hd, Wd, stride] that is the output's size or one row / column larger.
static inline int unet_upconv_dy_window(const char *what, uint32_t N, uint32_t H, uint32_t W, uint32_t Hd, uint32_t Wd, uint32_t stride,
                                        uint32_t off, uint32_t Cout) {
    LNH_REQUIRE(N && H && W && (uint64_t)N * H * W * 4 <= kUnetMaxPixels, LNH_ERR_INVALID_ARG,
                "%s: image [%u, %u, %u] (output of 1 .. 2^26 pixels)", what, N, H, W);
    LNH_REQUIRE(Hd >= 2 * H && Hd - 2 * H <= 1 && Wd >= 2 * W && Wd - 2 * W <= 1, LNH_ERR_INVALID_ARG,
                "%s: dy of %u x %u over an output of %u x %u (each 0 or 1 larger)", what, Hd, Wd, 2 * H, 2 * W);
    LNH_REQUIRE(stride % 8 == 0 && off % 8 == 0 && stride <= 2048 && (uint64_t)off + Cout <= stride, LNH_ERR_INVALID_ARG,
                "%s: channels [%u, %u + %u) of %u per pixel (offset and stride multiples of 8, stride up to 2048)", what, off, off, Cout,
                stride);
    return LNH_OK;
}

// The slices of a pixel-sliced weight gradient, from the shape alone: as many as 256-pixel pieces of the M pixels, as long as all
// slices' partials (slice_bytes each) fit the budget; the slice length L is then rounded up to the 32-pixel step and the count S
// taken again.
struct UnetSplit {
    uint32_t S;
    uint64_t L;
};
static inline UnetSplit unet_pixel_split(uint64_t M, uint64_t slice_bytes, uint64_t budget_bytes) {
    const uint64_t fit = budget_bytes / slice_bytes, pieces = (M + 255) / 256;
    const uint64_t S = pieces < fit ? pieces : (fit ? fit : 1);
    const uint64_t L = ((M + S - 1) / S + 31) / 32 * 32;
    return UnetSplit{(uint32_t)((M + L - 1) / L), L};
}
