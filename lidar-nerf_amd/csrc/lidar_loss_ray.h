// lidar_loss_ray.h — one ray of the default LiDAR loss (nerf/utils.py:712-746: L1 depth, MSE ray-drop, MSE intensity, all
// masked by the ground-truth ray-drop): its term of the sum and d loss / d (depth, image) of that ray.  k_lidar_loss
// (lidar_glue.hip) and the training forward tail (lidar_color.hip, k_color_forward_ray<true>) both call it: the two promise
// the same gradient bits, and they keep that promise by running the same fp32 expressions in the same order.  Built with
// -ffp-contract=off: the expressions are the bits.
#pragma once
#include "common.h"

namespace {

struct RayLoss {
    float l;                  // alpha_d |pd - gd| + alpha_r (pr - gr)^2 + alpha_i (pi - gi)^2 (not yet divided by N)
    float g_depth, g_image0, g_image1;  // d mean(l) / d depth, / d image[0:2], times gsc
};
// gt = (raydrop, intensity, depth) of the ray; N = rays of the batch (the mean's divisor); gsc = the gradient scale (1 if none)
__device__ __forceinline__ RayLoss lidar_loss_ray(float depth, float image0, float image1, float gt0, float gt1, float gt2,
                                                  uint32_t N, float a_d, float a_r, float a_i, float gsc) {
    const float gr = gt0, gi = gt1 * gr, gd = gt2 * gr;
    const float pr = image0, pi = image1 * gr, pd = depth * gr;
    const float dd = pd - gd, dr = pr - gr, di = pi - gi;
    RayLoss r;
    r.l = a_d * fabsf(dd) + a_r * dr * dr + a_i * di * di;
    const float inv = 1.0f / (float)N;
    const float sgn = dd > 0.0f ? 1.0f : (dd < 0.0f ? -1.0f : 0.0f);  // torch: sign(0) = 0
    r.g_depth = a_d * sgn * gr * inv * gsc;
    r.g_image0 = 2.0f * a_r * dr * inv * gsc;
    r.g_image1 = 2.0f * a_i * di * gr * inv * gsc;
    return r;
}

}  // namespace
