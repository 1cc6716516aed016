// composite_adjoint.h — the compositing adjoint of ONE dense ray, next to the walk it belongs to (transmittance.h): the two
// passes of k_lidar_composite_bwd (lidar_render.hip), which the training forward tail (lidar_color.hip,
// k_color_forward_ray<true>) runs as well, on the ray its wave has just composited.
//   c_i = g_ws + g_depth z_i + sum_k g_image_k rgb_ik,   total = sum_i w_i c_i   (pass 1),
//   dL/dalpha_i = T_i c_i - (total - sum_{j<=i} w_j c_j) / (1 - alpha_i + 1e-15)  (pass 2: the quotient form of
//   torch.cumprod's autograd),   grad_sigma_i = dL/dalpha_i * delta_i s exp(-delta_i s sigma_i).
// composite_adjoint_passes is the ONE statement of both passes: lane <-> sample mapping (64 samples a round, lane = sample),
// the order of every sum and every expression of the gradient.  Where a sample's alpha_i, T_i and c_i come from is the
// caller's source:
//   AdjointWalk   re-walks the ray from z, sigma and rgb in memory (the stand-alone kernel);
//   a stash       hands back what the forward walk of the same wave left in LDS (lidar_color.hip) — the same floats, since the
//                 forward formed them with the very definitions AdjointWalk calls (alpha_of, walk_step).
// grad_sigma therefore carries the same bits whichever kernel wrote it.
#pragma once
#include "transmittance.h"

namespace {

// one sample as a source hands it over.  A padding lane (i >= T) has alpha = 0 and a finite T.
struct AdjointSample {
    float alpha, om, T;  // alpha_i, 1 - alpha_i + eps, T_i  (w_i = alpha * T)
    float dsig;          // d alpha_i / d sigma_i = delta_i * s * exp(-delta_i s sigma_i)
    float c;             // c_i
};

// Src: begin() before each pass; load(base0) requests the kChunks rounds from sample base0 on; sample(u, i) hands over sample
// i = base0 + 64 u + lane, called once per round in ascending order (a source that walks keeps its carry that way).
// gs [T] out; gc [T, K] out (w_i g_image_k) or null.  Called by all 64 lanes of the wave that owns the ray.
// Src::kBatched (a source whose samples do not depend on one another): the rounds of a request are taken side by side —
// the same operations on the same operands, issued so that the kChunks prefix scans of a request overlap instead of
// following one another (a round past the end of the ray is computed on padding and dropped, where the serial form leaves
// the loop); what a tail wave pays for the adjoint is latency, and most of it was these scans in a row.
template <int K, class Src>
__device__ __forceinline__ void composite_adjoint_passes(Src &src, uint32_t T, const float (&gim)[K], int lane, float *gs,
                                                         float *gc) {
    // the gradient of sample i (i < T) from its inclusive prefix of w c
    auto emit = [&](uint32_t i, const AdjointSample &s, float cu, float w, float pref, float total) {
        const float suffix = total - pref;  // sum_{j>i} w_j c_j
        const float dalpha = s.T * cu - suffix / s.om;
        gs[i] = dalpha * s.dsig;
        if (gc) {
#pragma unroll
            for (int k = 0; k < K; k++) gc[(size_t)i * K + k] = w * gim[k];
        }
    };
    // pass 1: total = sum_i w_i c_i
    float total = 0.0f;
    src.begin();
    for (uint32_t base0 = 0; base0 < T; base0 += 64 * kChunks) {
        src.load(base0);
#pragma unroll
        for (int u = 0; u < kChunks; u++) {
            const uint32_t i = base0 + u * 64 + lane;
            const bool live = base0 + u * 64 < T;  // wave-uniform
            if constexpr (!Src::kBatched) {
                if (!live) break;
            }
            const AdjointSample s = src.sample(u, i);
            const float t = total + (i < T ? s.alpha * s.T * s.c : 0.0f);
            total = live ? t : total;
        }
    }
    total = wave_sum(total);

    // pass 2: prefix of w c, gradients
    float pref_carry = 0.0f;
    src.begin();
    for (uint32_t base0 = 0; base0 < T; base0 += 64 * kChunks) {
        src.load(base0);
        if constexpr (Src::kBatched) {
            AdjointSample s[kChunks];
            float cu[kChunks], w[kChunks], scan[kChunks];
#pragma unroll
            for (int u = 0; u < kChunks; u++) {  // (no branch in here: one block, seven independent scans)
                s[u] = src.sample(u, base0 + u * 64 + lane);
                cu[u] = base0 + u * 64 + lane < T ? s[u].c : 0.0f;
                w[u] = s[u].alpha * s[u].T;
                scan[u] = wave_scan_add(w[u] * cu[u], lane);
            }
#pragma unroll
            for (int u = 0; u < kChunks; u++) {
                const uint32_t i = base0 + u * 64 + lane;
                if (base0 + u * 64 >= T) break;  // wave-uniform
                const float pref = pref_carry + scan[u];  // inclusive prefix of w c
                if (i < T) emit(i, s[u], cu[u], w[u], pref, total);
                pref_carry = __shfl(pref, 63, 64);
            }
        } else {
#pragma unroll
            for (int u = 0; u < kChunks; u++) {
                const uint32_t i = base0 + u * 64 + lane;
                if (base0 + u * 64 >= T) break;  // wave-uniform
                const AdjointSample s = src.sample(u, i);
                const float cu = i < T ? s.c : 0.0f;
                const float w = s.alpha * s.T;
                const float wc = w * cu;
                const float pref = pref_carry + wave_scan_add(wc, lane);  // inclusive prefix of w c
                if (i < T) emit(i, s, cu, w, pref, total);
                pref_carry = __shfl(pref, 63, 64);
            }
        }
    }
}

// ---- the source that walks: zr, sr [T], cr [T, K] = merged depths, densities and colours of the ray in memory
template <int K>
struct AdjointWalk {
    static constexpr bool kBatched = false;  // (a round's T_i hangs on the carry of the round before)
    const float *zr, *sr, *cr;
    float sd, density_scale, gws, gdp, gim[K];
    uint32_t T;
    int lane;
    float carry;
    float zi[kChunks], zn[kChunks], sg[kChunks], ci[kChunks];

    __device__ __forceinline__ void begin() { carry = 1.0f; }
    // the chunks of both passes: z, sigma and c_i = g_ws + g_depth z_i + sum_k g_img_k rgb_ik
    __device__ __forceinline__ void load(uint32_t base0) {
        load_chunks(zr, base0, T, lane, zi, zn, [&](int u, uint32_t ic) {
            sg[u] = sr[ic];
            float c[K];
#pragma unroll
            for (int k = 0; k < K; k++) c[k] = cr[(size_t)ic * K + k];
            ci[u] = gws + gdp * zi[u];
#pragma unroll
            for (int k = 0; k < K; k++) ci[u] += gim[k] * c[k];
        });
    }
    __device__ __forceinline__ AdjointSample sample(int u, uint32_t i) {
        Alpha a;
        if (i < T) a = alpha_of(zi[u], zn[u], i + 1 < T, sg[u], sd, density_scale);
        const WalkStep s = walk_step(a.om, carry, lane);
        carry = walk_carry(s);
        return {a.alpha, a.om, s.T, a.delta * density_scale * a.e, ci[u]};
    }
};

}  // namespace
