// transmittance.h — the one walk along a ray that every LiDAR compositing kernel takes (renderer.py:233-243 on the dense
// [N, T] samples, raymarching.cu:577-772 semantics on the marcher's ragged ones).  One 64-lane wave owns one ray and takes
// its samples 64 at a time (lane = sample within the round):
//   alpha_i = 1 - exp(-delta_i s sigma_i),   T_i = prod_{j<i} (1 - alpha_j (+ 1e-15)),   w_i = alpha_i T_i,
// T_i out of an inclusive product scan across the lanes, shifted by one lane, times a scalar carry from the rounds before.
// lidar_render.hip, lidar_field.hip, lidar_color.hip and raymarch.hip promise the same bits for the same samples; they keep
// that promise by all using the definitions below.  Built with -ffp-contract=off: the expressions are the bits.
#pragma once
#include "common.h"

namespace {

constexpr float kTransEps = 1e-15f;  // renderer.py:189,241: keeps 1 - alpha away from an exact 0 in the cumprod
// A plain loop over the rounds pays one dependent HBM round trip per 64 samples (13 at 832 samples: the one-wave-per-ray
// kernels ran at that latency, not at bandwidth).  They request kChunks rounds at once and scan them from registers.
constexpr int kChunks = 7;

// ---- the alpha rule of the dense samples.  The defaults are a padding lane (i >= T): it contributes alpha = 0, om = 1.
struct Alpha {
    float delta = 0.0f, e = 1.0f, alpha = 0.0f, om = 1.0f;  // e = exp(-delta s sigma), om = 1 - alpha + eps
};
// zn = z[i + 1], ignored for the last sample of the ray (has_next == false), whose delta is the ray's sample_dist
__device__ __forceinline__ Alpha alpha_of(float zi, float zn, bool has_next, float sigma, float sample_dist,
                                          float density_scale) {
    Alpha a;
    a.delta = has_next ? (zn - zi) : sample_dist;
    a.e = expf(-a.delta * density_scale * sigma);
    a.alpha = 1.0f - a.e;
    a.om = 1.0f - a.alpha + kTransEps;
    return a;
}

// ---- one round of the walk.  om: this lane's 1 - alpha (dense: + eps, ragged: none); carry: T in front of lane 0.
struct WalkStep {
    float T, Tn;  // T_i and T_{i+1} of this lane's sample: w_i = alpha_i * T (never (alpha * carry) * excl)
};
__device__ __forceinline__ WalkStep walk_step(float om, float carry, int lane) {
    const float incl = wave_scan_mul(om, lane);
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 1.0f;
    return {carry * excl, carry * incl};
}
// T in front of the next round: T_{i+1} of lane 63 = carry * incl[63] (the carry is wave-uniform, so this is the one IEEE
// product `carry *= incl[63]` is).  The dense kernels take it every round; the ragged ones leave on their stop ballot first.
__device__ __forceinline__ float walk_carry(const WalkStep &s) { return __shfl(s.Tn, 63, 64); }

// ---- kChunks rounds of a dense ray requested at once: zi[u] = z[i], zn[u] = z[i + 1] for i = base0 + 64 u + lane, with
// the indices clamped into the row (a padding lane reads sample 0, the last sample reads itself as its successor).
// more(u, ic) loads whatever else the site needs of sample ic.
template <class More>
__device__ __forceinline__ void load_chunks(const float *__restrict__ zr, uint32_t base0, uint32_t T, uint32_t lane,
                                            float (&zi)[kChunks], float (&zn)[kChunks], More &&more) {
#pragma unroll
    for (int u = 0; u < kChunks; u++) {
        const uint32_t i = base0 + u * 64 + lane, ic = i < T ? i : 0, in = i + 1 < T ? i + 1 : ic;
        zi[u] = zr[ic];
        zn[u] = zr[in];
        more(u, ic);
    }
}

// ---- one sample of a ragged ray (row i of the marcher's buffers): alpha = 1 - exp(-sigma dt), z = (xyz - o) . d the
// distance along the unit ray, the K features.  A lane without a sample (in == false) holds zeros.  The training
// compositors and the alive-ray evaluation both load through here: a sample carries the same bits on both paths.
template <int K>
struct RaySample {
    float alpha = 0.0f, dt = 0.0f, z = 0.0f, f[K] = {};
};
template <int K>
__device__ __forceinline__ RaySample<K> load_ray_sample(bool in, size_t i, const float *__restrict__ sigmas,
                                                        const float *__restrict__ feats,
                                                        const float *__restrict__ deltas,
                                                        const float *__restrict__ xyzs, float ox, float oy, float oz,
                                                        float dx, float dy, float dz) {
    RaySample<K> s;
    if (in) {
        s.dt = deltas[i * 2];
        s.alpha = 1.0f - expf(-sigmas[i] * s.dt);
        s.z = (xyzs[i * 3] - ox) * dx + (xyzs[i * 3 + 1] - oy) * dy + (xyzs[i * 3 + 2] - oz) * dz;
#pragma unroll
        for (int k = 0; k < K; k++) s.f[k] = feats[i * K + k];
    }
    return s;
}

}  // namespace
