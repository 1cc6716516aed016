// nvs_ssim_tile.h — the indexing and the arithmetic of the 1-D SSIM of eval_nvs.hip that one workgroup applies to one tile,
// written so that it also compiles as plain C++: tools/nvs_ssim_tile_host.cpp runs exactly this code on the host, under the
// address and undefined-behaviour sanitizers, with every array allocated at its exact size.  Nothing here launches anything.
//
// The evaluated sequence is the window of h x w pixels at (r0, c0) of an H x W image, row-major: element p of n = h * w is the
// pixel (r0 + p / w, c0 + p % w).  Position q of the n - 6 SSIM positions covers the elements q .. q + 6.  Tile t owns the
// positions [t * kNvsTile, min(n - 6, (t + 1) * kNvsTile)) and stages the elements [t * kNvsTile, min(n, t * kNvsTile +
// kNvsStage)): its positions' windows, the 6-element halo on the right included (the left one belongs to the tile before).
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include "common.h"
#define NVS_HD __host__ __device__ __forceinline__
#else
#define NVS_HD inline
#endif

constexpr uint32_t kNvsWin = 7, kNvsHalo = kNvsWin - 1;
constexpr uint32_t kNvsTile = 256, kNvsStage = kNvsTile + kNvsHalo;

struct NvsSeq {
    uint32_t r0, c0, h, w, W, n;  // the window, the image's row pitch, n = h * w (0: no sequence)
};

// numpy's in-place clamp of compute_depth_metrics (eval.py:81-84): a NaN stays a NaN
NVS_HD float nvs_clamp_depth(float x) { return x < 1e-3f ? 1e-3f : (x > 80.0f ? 80.0f : x); }

// the pixel index (row * W + col) of sequence element p < n
NVS_HD uint32_t nvs_seq_pixel(const NvsSeq &s, uint32_t p) {
    const uint32_t r = p / s.w;
    return (s.r0 + r) * s.W + s.c0 + (p - r * s.w);
}

// number of SSIM positions of the sequence, and of the tiles that own one
NVS_HD uint32_t nvs_positions(uint32_t n) { return n >= kNvsWin ? n - kNvsHalo : 0u; }
NVS_HD uint32_t nvs_tiles(uint32_t n) { return (nvs_positions(n) + kNvsTile - 1) / kNvsTile; }
// elements tile t stages / positions it owns (0 for a tile behind the last)
NVS_HD uint32_t nvs_tile_staged(uint32_t n, uint32_t t) {
    const uint64_t first = (uint64_t)t * kNvsTile;
    if (first >= nvs_positions(n)) return 0u;
    return (uint32_t)((n - first) < kNvsStage ? (n - first) : kNvsStage);
}
NVS_HD uint32_t nvs_tile_positions(uint32_t n, uint32_t t) {
    const uint64_t first = (uint64_t)t * kNvsTile, all = nvs_positions(n);
    if (first >= all) return 0u;
    return (uint32_t)((all - first) < kNvsTile ? (all - first) : kNvsTile);
}

// S of one position: x, y point at the window's 7 staged elements.  skimage.metrics.structural_similarity's defaults on a
// 1-D signal: uniform window of 7, sample covariance (7 / 6), C1 = (0.01 R)^2, C2 = (0.03 R)^2.  The five moments are fp64 sums
// of the float32 values, left to right (a product of two float32 is exact in fp64); one rounded operation per operator
// (-ffp-contract=off), so two identical windows give A1 == B1 and A2 == B2 bit for bit and S == 1 exactly.
NVS_HD double nvs_ssim_at(const float *x, const float *y, double c1, double c2) {
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (uint32_t j = 0; j < kNvsWin; j++) {
        const double a = (double)x[j], b = (double)y[j];
        sx += a;
        sy += b;
        sxx += a * a;
        syy += b * b;
        sxy += a * b;
    }
    const double np = (double)kNvsWin, cov_norm = np / (np - 1.0);
    const double ux = sx / np, uy = sy / np, uxx = sxx / np, uyy = syy / np, uxy = sxy / np;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
    const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
    return (a1 * a2) / (b1 * b2);
}

// C1 and C2 from the float32 minimum and maximum of the clamped ground truth (data_range is their float32 difference, as
// NumPy forms gt.max() - gt.min() of a float32 array)
NVS_HD void nvs_ssim_constants(float gmin, float gmax, double &c1, double &c2) {
    const double range = (double)(gmax - gmin);
    c1 = (0.01 * range) * (0.01 * range);
    c2 = (0.03 * range) * (0.03 * range);
}
