// pano_geom.h — the one copy of the range-image geometry, both ways.
// Back-projection (convert.py:207-223, pano_to_lidar_with_intensities): pixel (row j, column i) of an H x W range image with
// depth d -> the point in the sensor frame.  Used by k_pano_to_lidar (convert.hip) and by the fused points meter
// (eval_points.hip), whose clouds must equal convert.pano_to_lidar's bit for bit.
// Projection (convert.py:99-160, lidar_to_pano_with_intensities): a point in the sensor frame -> its pixel.  Used by the three
// projections of convert.hip and by the TSDF integration (tsdf.hip), so that a lattice point and a LiDAR return project alike.
#pragma once
#include "common.h"

struct PanoGeom {
    float pi_f;        // float32(np.pi)
    float down_rad;    // float32(fov_down / 180 * pi)
    float col_step;    // float32(2 pi / W)
    float row_step;    // float32(fov / 180 * pi / H)
    float max_depth;
    uint32_t H, W;
};
static inline PanoGeom pano_geom(uint32_t H, uint32_t W, float fov_up, float fov, float max_depth) {
    constexpr double kPi = 3.14159265358979323846;
    PanoGeom g;
    g.pi_f = (float)kPi;
    g.down_rad = (float)(((double)fov - (double)fov_up) / 180.0 * kPi);
    g.col_step = (float)(2.0 * kPi / (double)W);
    g.row_step = (float)((double)fov / 180.0 * kPi / (double)H);
    g.max_depth = max_depth;
    g.H = H;
    g.W = W;
    return g;
}

// atan2 is evaluated in double and rounded to float, which reproduces a correctly-rounded atan2f
#ifdef LNH_PANO_ATAN2_F32
// timing probe of tools/bench_tsdf.py only (what the double costs): NOT the contract, the pixels differ
__device__ __forceinline__ float atan2_rn(float y, float x) { return atan2f(y, x); }
#else
__device__ __forceinline__ float atan2_rn(float y, float x) { return (float)atan2((double)y, (double)x); }
#endif

// Point (x, y, z) in the sensor frame -> pixel: the reference's float32 arithmetic.  Returns the row-major pixel id, or kNoPixel
// for a point the reference skips (dist >= max_depth, outside the image; dist == 0).  kWrapColumn is the one difference the TSDF
// integration asks for: a column that rounds to W is column 0 (the seam behind the sensor), where the reference drops the point.
constexpr uint32_t kNoPixel = 0xffffffffu;
template <bool kWrapColumn>
__device__ __forceinline__ uint32_t pano_pixel_xyz(float x, float y, float z, const PanoGeom &g, float &dist) {
    dist = sqrtf(x * x + y * y + z * z);  // np.linalg.norm over 3 float32 values
    if (!(dist < g.max_depth) || !(dist > 0.0f)) return kNoPixel;  // reference: `if dist >= max_depth: continue`
    const float beta = g.pi_f - atan2_rn(y, x);
    const float alpha = atan2_rn(z, sqrtf(x * x + y * y)) + g.down_rad;
    float cf = rintf(beta / g.col_step);                       // Python round(): half to even
    const float rf = rintf((float)g.H - alpha / g.row_step);
    if (kWrapColumn && cf == (float)g.W) cf = 0.0f;
    if (!(rf >= 0.0f) || !(cf >= 0.0f) || rf >= (float)g.H || cf >= (float)g.W) return kNoPixel;
    return (uint32_t)rf * g.W + (uint32_t)cf;
}

// convert.py:207-217: float32 index grids; W/2, W, H are Python scalars (weak), 2*np.pi and 180 likewise
__device__ __forceinline__ void pano_point(uint32_t j, uint32_t i, uint32_t H, uint32_t W, float fov_up, float fov, float d,
                                           float &x, float &y, float &z) {
    constexpr double kPanoPi = 3.14159265358979323846;
    const float beta = -((float)i - (float)(W / 2.0)) / (float)W * 2.0f * (float)kPanoPi;
    const float alpha = (fov_up - (float)j / (float)H * fov) / 180.0f * (float)kPanoPi;
    const float ca = cosf(alpha), sa = sinf(alpha), cb = cosf(beta), sb = sinf(beta);
    x = ca * cb * d;
    y = ca * sb * d;
    z = sa * d;
}
