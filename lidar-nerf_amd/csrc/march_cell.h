// march_cell.h — what a marcher sees at one ray parameter: the step length, the occupancy cell and the walk out of an empty
// cell (raymarching.cu:51-95, 379-439).  Shared by the training marcher (raymarch.hip) and the alive-ray evaluation marcher
// (lidar_infer.hip): both walk the SAME lattice with the SAME probes, which is what makes their samples bit-identical.
// Needs -ffp-contract=off like everything derived from float math that must match the CPU oracle (see raymarch.hip).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }
__device__ __forceinline__ float signf(float x) { return copysignf(1.0f, x); }

// raymarching.cu:71-95 — 10-bit-per-axis Morton code via magic-number bit spreading
__device__ __forceinline__ uint32_t spread3(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton_encode(uint32_t x, uint32_t y, uint32_t z) {
    return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2);
}
__device__ __forceinline__ uint32_t compact3(uint32_t x) {
    x &= 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// raymarching.cu:51-69
__device__ __forceinline__ int mip_from_pos(float x, float y, float z, float max_cascade) {
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)e));
}
__device__ __forceinline__ int mip_from_dt(float dt, float H, float max_cascade) {
    const float mx = (float)((double)(dt * H) * 0.5);
    int e;
    frexpf(mx, &e);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)e));
}
// raymarching.cu:397-405: product in double, clamp in float, truncate
__device__ __forceinline__ int cell_coord(float x, float mip_rbound, uint32_t H) {
    const double v = 0.5 * (double)fmaf(x, mip_rbound, 1.0f) * (double)H;
    return (int)clampf((float)v, 0.0f, (float)(H - 1));
}

struct Probe {
    float x, y, z, dt, t_next, tt;
    uint32_t index;
    bool occ;
};

struct MarchRay {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
};

// The step length at parameter t (raymarching.cu:389): the marcher only ever moves by this amount, occupied or not.
__device__ __forceinline__ float march_dt(float t, float dt_gamma, float dt_min, float dt_max) {
    return clampf(t * dt_gamma, dt_min, dt_max);
}

// What the marcher sees at parameter t (raymarching.cu:379-430): the clamped position, its cell's occupancy bit and — for
// an empty cell — tt, the parameter at which the ray leaves that cell.
__device__ __forceinline__ Probe probe_cell(const MarchRay &r, float t, const uint8_t *__restrict__ grid, float bound,
                                            float dt_gamma, float dt_min, float dt_max, uint32_t C, uint32_t H, float rH,
                                            float H3) {
    Probe p;
    p.x = clampf(fmaf(t, r.dx, r.ox), -bound, bound);
    p.y = clampf(fmaf(t, r.dy, r.oy), -bound, bound);
    p.z = clampf(fmaf(t, r.dz, r.oz), -bound, bound);
    p.dt = march_dt(t, dt_gamma, dt_min, dt_max);
    const int level = max(mip_from_pos(p.x, p.y, p.z, (float)C), mip_from_dt(p.dt, (float)H, (float)C));
    const float mip_bound = fminf(scalbnf(1.0f, level), bound);
    const float mip_rbound = 1 / mip_bound;
    const int nx = cell_coord(p.x, mip_rbound, H), ny = cell_coord(p.y, mip_rbound, H),
              nz = cell_coord(p.z, mip_rbound, H);
    p.index = (uint32_t)((float)level * H3 + (float)morton_encode((uint32_t)nx, (uint32_t)ny, (uint32_t)nz));
    p.occ = (grid[p.index >> 3] & (1u << (p.index & 7u))) != 0;
    p.t_next = p.tt = t;
    if (!p.occ) {
        const float tx = (((nx + 0.5f + 0.5f * signf(r.dx)) * rH * 2 - 1) * mip_bound - p.x) * r.rdx;
        const float ty = (((ny + 0.5f + 0.5f * signf(r.dy)) * rH * 2 - 1) * mip_bound - p.y) * r.rdy;
        const float tz = (((nz + 0.5f + 0.5f * signf(r.dz)) * rH * 2 - 1) * mip_bound - p.z) * r.rdz;
        p.tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
    }
    return p;
}

// One decision of the serial marcher at parameter t (raymarching.cu:379-439): probe_cell + the walk out of an empty cell.
__device__ __forceinline__ Probe probe(const MarchRay &r, float t, const uint8_t *__restrict__ grid, float bound,
                                       float dt_gamma, float dt_min, float dt_max, uint32_t C, uint32_t H, float rH,
                                       float H3) {
    Probe p = probe_cell(r, t, grid, bound, dt_gamma, dt_min, dt_max, C, H, rH, H3);
    if (!p.occ) {
        do {
            t += march_dt(t, dt_gamma, dt_min, dt_max);
        } while (t < p.tt);
        p.t_next = t;
    }
    return p;
}

}  // namespace
