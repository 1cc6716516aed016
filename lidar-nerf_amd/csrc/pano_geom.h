// pano_geom.h — the one copy of the range-image back-projection (convert.py:207-223, pano_to_lidar_with_intensities):
// pixel (row j, column i) of an H x W range image with depth d -> the point in the sensor frame.  Used by k_pano_to_lidar
// (convert.hip) and by the fused points meter (eval_points.hip), whose clouds must equal convert.pano_to_lidar's bit for bit.
#pragma once
#include "common.h"

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
