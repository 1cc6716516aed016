// lidar_infer.hip — occupancy-grid EVALUATION of LiDAR rays as an alive-ray loop (gfx950).
// The lineage's inference renderer (raymarching.cu:808-928 march_rays, 966-1053 composite_rays; raymarching.py:362-512)
// marches a few samples per alive ray, shades them, composites them, drops the rays that saturated or left the box and
// repeats on the survivors.  raymarch.hip keeps the RGB template of those two kernels (lane-per-ray serial walks, three
// channels, relative depth, T = 1 - weights_sum, survivors compacted by the caller).  The three kernels here are the LiDAR
// renderer's own round:
//   k_lidar_march_rays      one WAVE per alive ray on the lattice of k_march_rays_train (march_cell.h: same probes, same
//                           comparisons), at most n_step samples from the ray's saved parameter; IT stores the resume
//                           parameter, so a ray's samples over all rounds are bit for bit the prefix of what the training
//                           marcher emits for it without perturbation;
//   k_lidar_composite_rays  one sub-wave GROUP of lanes per ray, one lane per sample: the arithmetic and the stop rule of
//                           k_lidar_composite_ragged_fwd (K channels, absolute depth sum w (xyz - o) . d, carried
//                           transmittance), accumulated in place into per-ray state;
//   k_alive_compact         the surviving ray ids, in slot order, into the other half of a ping-pong list + their count.
// The alive count lives in device memory: launches are sized by a host upper bound and every kernel clips it to the count.
// No float atomics anywhere: two runs give the same bits.  Built with -ffp-contract=off (see raymarch.hip).
#include "common.h"
#include "march_cell.h"
#include "transmittance.h"

namespace {

constexpr uint32_t kInferRaysPerGroup = 16;  // waves (= rays) per workgroup of the marcher, as in k_march_rays_train

__device__ __forceinline__ float lidar_infer_left_box() { return __builtin_inff(); }  // resume mark: t < far never holds

// rays_alive[0 .. n_alive) are ray ids; slot n owns sample rows [n * n_step, (n + 1) * n_step).
__global__ void __launch_bounds__(64 * kInferRaysPerGroup)
k_lidar_march_rays(uint32_t n_alive_max, uint32_t n_step, uint32_t N, const int32_t *__restrict__ alive_count,
                   const int32_t *__restrict__ rays_alive, float *__restrict__ rays_t, int32_t *__restrict__ rays_steps,
                   const float *__restrict__ rays_o, const float *__restrict__ rays_d, const uint8_t *__restrict__ grid,
                   float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                   const float *__restrict__ fars, float *__restrict__ xyzs, float *__restrict__ deltas,
                   int32_t *__restrict__ rays, int32_t *__restrict__ samples_total) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t n = blockIdx.x * kInferRaysPerGroup + wv;  // row of the round's ray table (wave-uniform)
    if (n >= N) return;
    const int32_t cnt = alive_count[0];
    const uint32_t n_alive = min(cnt > 0 ? (uint32_t)cnt : 0u, n_alive_max);
    const uint32_t index = n < n_alive ? (uint32_t)rays_alive[n] : N;
    if (index >= N) {
        // not a ray of this round (beyond the alive count, or not an id): an empty table row, no sample in its slots
        if (lane == 0) { rays[n * 3] = 0; rays[n * 3 + 1] = 0; rays[n * 3 + 2] = 0; }
        if (n < n_alive_max)
            for (uint32_t i = lane; i < n_step * 2; i += 64) deltas[(size_t)n * n_step * 2 + i] = 0.0f;
        return;
    }
    MarchRay r;
    r.ox = rays_o[index * 3]; r.oy = rays_o[index * 3 + 1]; r.oz = rays_o[index * 3 + 2];
    r.dx = rays_d[index * 3]; r.dy = rays_d[index * 3 + 1]; r.dz = rays_d[index * 3 + 2];
    r.rdx = 1 / r.dx; r.rdy = 1 / r.dy; r.rdz = 1 / r.dz;
    const float rH = 1 / (float)H, H3 = (float)(H * H * H);
    const float far = fars[index];
    const float SQRT3 = 1.7320508075688772f;
    const float dt_min = 2 * SQRT3 / max_steps;
    const float dt_max = 2 * SQRT3 * (float)(1 << (C - 1)) / H;
    const float t0 = rays_t[index];
    const uint32_t before_round = min((uint32_t)max(rays_steps[index], 0), max_steps);
    const uint32_t budget = min(n_step, max_steps - before_round);  // (the training marcher emits at most max_steps per ray)
    const unsigned long long below = (1ull << lane) - 1;

    // The walk of k_march_rays_train's chunk(), 64 lattice points at a time, with this round's budget in the place of
    // max_steps; `full` = the budget is used up (the ray resumes behind its last sample), `ended` = the walk passed `far`.
    float t_base = t0, pending_tt = 0.0f, last_t = t0;
    bool pending = false, full = budget == 0, ended = false;
    uint32_t emitted = 0;
    const size_t row0 = (size_t)n * n_step;
    while (!full && !ended) {
        float t = t_base;
#pragma unroll 8
        for (uint32_t i = 0; i < 63; i++)
            if (i < lane) t += march_dt(t, dt_gamma, dt_min, dt_max);
        const float t_last = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), 63));
        t_base = t_last + march_dt(t_last, dt_gamma, dt_min, dt_max);
        const bool valid_l = t < far;
        const unsigned long long valid = __ballot(valid_l);
        Probe p;
        p.occ = false;
        p.tt = t;
        p.x = p.y = p.z = p.dt = 0.0f;
        if (valid_l) p = probe_cell(r, t, grid, bound, dt_gamma, dt_min, dt_max, C, H, rH, H3);
        const unsigned long long occm = __ballot(valid_l && p.occ);
        unsigned long long emit = 0;
        uint32_t pos = 0;
        if (pending) {  // still inside the empty cell an earlier chunk met
            const unsigned long long ge = __ballot(t >= pending_tt);
            if (!ge) {
                if (valid != ~0ull) ended = true;
                continue;
            }
            pos = (uint32_t)__builtin_ctzll(ge);
            pending = false;
        }
        while (pos < 64) {
            if (!((valid >> pos) & 1)) { ended = true; break; }
            if (emitted + (uint32_t)__builtin_popcountll(emit) >= budget) { full = true; break; }
            if ((occm >> pos) & 1) {  // a run of occupied lattice points
                const unsigned long long rest = ~occm >> pos;
                const uint32_t run = rest ? (uint32_t)__builtin_ctzll(rest) : 64 - pos;
                emit |= (run >= 64 ? ~0ull : ((1ull << run) - 1)) << pos;
                pos += run;
            } else {                  // empty: on to the first t >= tt
                const float tt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p.tt), (int)pos));
                const unsigned long long ge = __ballot(t >= tt) & ~((2ull << pos) - 1);
                if (!ge) { pending = true; pending_tt = tt; break; }
                pos = (uint32_t)__builtin_ctzll(ge);
            }
        }
        while (emitted + (uint32_t)__builtin_popcountll(emit) > budget) {  // a run went past the budget: keep the front
            emit &= ~(1ull << (63 - __builtin_clzll(emit)));
            full = true;
        }
        if (emitted + (uint32_t)__builtin_popcountll(emit) >= budget) full = true;
        if (valid != ~0ull) ended = true;
        if (!emit) continue;
        const float t_after = t + p.dt;  // (= the next lattice point: the serial walk's `t += dt`)
        const unsigned long long before = emit & below;
        const int prev = before ? 63 - (int)__builtin_clzll(before) : 0;
        const float prev_after = __shfl(t_after, prev, 64);
        if ((emit >> lane) & 1) {
            const size_t row = row0 + emitted + (uint32_t)__builtin_popcountll(before);
            xyzs[row * 3] = p.x; xyzs[row * 3 + 1] = p.y; xyzs[row * 3 + 2] = p.z;
            deltas[row * 2] = p.dt;
            deltas[row * 2 + 1] = t_after - (before ? prev_after : last_t);
        }
        last_t = __shfl(t_after, 63 - (int)__builtin_clzll(emit), 64);
        emitted += (uint32_t)__builtin_popcountll(emit);
    }
    // the slots this ray did not fill carry no sample (delta == 0, the lineage's end-of-ray mark)
    for (uint32_t i = emitted * 2 + lane; i < n_step * 2; i += 64) deltas[row0 * 2 + i] = 0.0f;
    if (lane == 0) {
        rays[n * 3] = (int32_t)index;
        rays[n * 3 + 1] = (int32_t)row0;
        rays[n * 3 + 2] = (int32_t)emitted;
        const uint32_t total = before_round + emitted;
        rays_steps[index] = (int32_t)total;
        // resume exactly behind the last sample — or nowhere: the walk ended, or the ray has its max_steps samples
        rays_t[index] = (emitted == n_step && total < max_steps) ? last_t : lidar_infer_left_box();
        if (samples_total && emitted) atomicAdd(samples_total, (int32_t)emitted);
    }
}

// One group of W lanes (W a power of two, 1 .. 64) per slot of the round, one lane per sample.
template <int K>
__global__ void __launch_bounds__(256)
k_lidar_composite_rays(uint32_t n_alive_max, uint32_t n_step, uint32_t N, uint32_t W, float T_thresh,
                       const int32_t *__restrict__ alive_count, int32_t *__restrict__ rays_alive,
                       const float *__restrict__ rays_t, const int32_t *__restrict__ rays,
                       const float *__restrict__ sigmas, const float *__restrict__ feats,
                       const float *__restrict__ deltas, const float *__restrict__ xyzs,
                       const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                       float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
                       float *__restrict__ trans) {
    const uint32_t lane = threadIdx.x & 63, gl = lane & (W - 1), gshift = lane & ~(W - 1);
    const uint32_t n = (blockIdx.x * 256 + threadIdx.x) / W;  // slot
    const int32_t cnt = alive_count[0];
    const uint32_t n_alive = min(cnt > 0 ? (uint32_t)cnt : 0u, n_alive_max);
    const bool slot = n < n_alive;
    const uint32_t nc = slot ? n : 0;
    const uint32_t index = slot ? (uint32_t)rays[nc * 3] : N, offset = (uint32_t)rays[nc * 3 + 1];
    uint32_t count = (uint32_t)rays[nc * 3 + 2];
    const bool ray = slot && index < N && rays_alive[nc] == (int32_t)index;  // (a row the marcher wrote for this very slot)
    if (!ray || (uint64_t)offset + count > (uint64_t)n_alive_max * n_step) count = 0;
    const uint32_t ic = ray ? index : 0;
    const float ox = rays_o[ic * 3], oy = rays_o[ic * 3 + 1], oz = rays_o[ic * 3 + 2];
    const float dx = rays_d[ic * 3], dy = rays_d[ic * 3 + 1], dz = rays_d[ic * 3 + 2];
    const unsigned long long gmask = W >= 64 ? ~0ull : ((1ull << W) - 1);
    float acc[K], ws = 0, d = 0;
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = 0;
    float Tc = ray ? trans[ic] : 1.0f;  // transmittance in front of this chunk
    bool stopped = false;
    for (uint32_t base = 0; base < n_step; base += W) {  // (trip count uniform over the wave: groups idle past their count)
        const uint32_t step = base + gl;
        const bool in = !stopped && step < count;
        const size_t i = (size_t)offset + (in ? step : 0);
        const RaySample<K> s = load_ray_sample<K>(in, i, sigmas, feats, deltas, xyzs, ox, oy, oz, dx, dy, dz);
        // the sample load is the training compositors'; the scan is not walk_step: W is a run-time width inside a wave
        float incl = 1.0f - s.alpha;  // multiplicative scan inside the group
        for (uint32_t o = 1; o < W; o <<= 1) {
            const float u = __shfl_up(incl, o, 64);
            if (gl >= o) incl *= u;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (gl == 0) excl = 1.0f;
        const float T = Tc * excl, Tn = Tc * incl;  // T_i, T_{i+1}
        // stop after the first sample that takes T below the threshold
        const unsigned long long stop = (__ballot(in && Tn < T_thresh) >> gshift) & gmask;
        const uint32_t last = stop ? (uint32_t)__builtin_ctzll(stop) : W - 1;
        const float w = (in && gl <= last) ? s.alpha * T : 0.0f;
        ws += w;
        d += w * s.z;
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] += w * s.f[k];
        const float Tnext = __shfl(Tn, (int)(gshift + last), 64);
        if (!stopped) Tc = Tnext;
        if (stop) stopped = true;
    }
    for (uint32_t o = W >> 1; o > 0; o >>= 1) {  // sums over the group
        ws += __shfl_xor(ws, o, 64);
        d += __shfl_xor(d, o, 64);
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if (gl == 0 && slot) {
        if (ray) {
            if (count) {
                weights_sum[index] += ws;
                depth[index] += d;
#pragma unroll
                for (int k = 0; k < K; k++) image[index * K + k] += acc[k];
                trans[index] = Tc;
            }
            // dead: saturated, a short round (the walk ended inside it), or the marcher's mark (no resume parameter)
            const bool dead = stopped || count < n_step || !(rays_t[index] < lidar_infer_left_box());
            if (dead) rays_alive[n] = -1;
        } else {
            rays_alive[n] = -1;
        }
    }
}

// Stable compaction by ONE workgroup: chunks of 1024 slots in order, ballot + popcount inside a wave, the 16 wave totals
// through LDS.  (A render call works on max_ray_batch = 4096 rays at a time: four trips.  Nothing here depends on the
// order workgroups arrive in, so the list — and with it every later round — is the same on every run.)
__global__ void __launch_bounds__(1024)
k_alive_compact(uint32_t n_alive_max, const int32_t *__restrict__ alive_count, const int32_t *__restrict__ rays_alive,
                int32_t *__restrict__ rays_alive_out, int32_t *__restrict__ alive_count_out) {
    __shared__ uint32_t s_wave[16];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int32_t cnt = alive_count[0];
    const uint32_t n_in = min(cnt > 0 ? (uint32_t)cnt : 0u, n_alive_max);
    uint32_t running = 0;
    for (uint32_t base = 0; base < n_in; base += 1024) {  // (n_in is the same for every thread: uniform trip count)
        const uint32_t i = base + threadIdx.x;
        const int32_t v = i < n_in ? rays_alive[i] : -1;
        const bool keep = v >= 0;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wv] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t c = s_wave[k];
            if (k < wv) before += c;
            total += c;
        }
        if (keep) rays_alive_out[running + before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1))] = v;
        running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) alive_count_out[0] = (int32_t)running;
}

}  // namespace

extern "C" {

int lnh_lidar_march_rays(uint32_t n_alive_max, uint32_t n_step, uint32_t N, const int32_t *alive_count,
                         const int32_t *rays_alive, float *rays_t, int32_t *rays_steps, const float *rays_o,
                         const float *rays_d, const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps,
                         uint32_t C, uint32_t H, const float *fars, float *xyzs, float *deltas, int32_t *rays,
                         int32_t *samples_total, lnh_stream_t stream) {
    LNH_REQUIRE(n_step >= 1, LNH_ERR_INVALID_ARG, "lidar_march_rays: n_step must be at least 1");
    LNH_REQUIRE(rays_t && rays_steps, LNH_ERR_INVALID_ARG, "lidar_march_rays: null ray state (rays_t / rays_steps)");
    LNH_REQUIRE(alive_count && rays_alive && rays_o && rays_d && grid && fars && xyzs && deltas && rays, LNH_ERR_INVALID_ARG,
                "lidar_march_rays: null pointer");
    LNH_REQUIRE(C >= 1 && C <= 8 && H >= 1 && H <= 1024 && max_steps >= 1, LNH_ERR_INVALID_ARG,
                "lidar_march_rays: bad cascade / grid size / max_steps");
    LNH_REQUIRE(n_alive_max <= N && (uint64_t)n_alive_max * n_step <= 0x7fffffffull, LNH_ERR_INVALID_ARG,
                "lidar_march_rays: n_alive_max must not exceed N, n_alive_max * n_step must fit 31 bits");
    if (N == 0) return LNH_OK;
    LNH_LAUNCH(k_lidar_march_rays, dim3(div_up(N, kInferRaysPerGroup)), dim3(64 * kInferRaysPerGroup), 0,
               (hipStream_t)stream, n_alive_max, n_step, N, alive_count, rays_alive, rays_t, rays_steps, rays_o, rays_d, grid,
               bound, dt_gamma, max_steps, C, H, fars, xyzs, deltas, rays, samples_total);
    return lnh_check_launch("lnh_lidar_march_rays");
}

int lnh_lidar_composite_rays(uint32_t n_alive_max, uint32_t n_step, uint32_t N, uint32_t K, float T_thresh,
                             const int32_t *alive_count, int32_t *rays_alive, const float *rays_t, const int32_t *rays,
                             const float *sigmas, const float *feats, const float *deltas, const float *xyzs,
                             const float *rays_o, const float *rays_d, float *weights_sum, float *depth, float *image,
                             float *transmittance, lnh_stream_t stream) {
    LNH_REQUIRE(n_step >= 1, LNH_ERR_INVALID_ARG, "lidar_composite_rays: n_step must be at least 1");
    LNH_REQUIRE(K >= 1 && K <= 3, LNH_ERR_UNSUPPORTED, "lidar_composite_rays: K must be 1, 2 or 3 (got %u)", K);
    LNH_REQUIRE(weights_sum && depth && image && transmittance, LNH_ERR_INVALID_ARG,
                "lidar_composite_rays: null ray state (weights_sum / depth / image / transmittance)");
    LNH_REQUIRE(alive_count && rays_alive && rays_t && rays && sigmas && feats && deltas && xyzs && rays_o && rays_d,
                LNH_ERR_INVALID_ARG, "lidar_composite_rays: null pointer");
    LNH_REQUIRE(n_alive_max <= N && (uint64_t)n_alive_max * n_step <= 0x7fffffffull, LNH_ERR_INVALID_ARG,
                "lidar_composite_rays: n_alive_max must not exceed N, n_alive_max * n_step must fit 31 bits");
    if (n_alive_max == 0) return LNH_OK;
    uint32_t W = 1;  // lanes per ray: the power of two that holds a round's samples, a wave at most
    while (W < n_step && W < 64) W <<= 1;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t blocks = div_up((uint64_t)n_alive_max * W, 256);
#define LNH_INFER_COMPOSITE(KK)                                                                                        \
    LNH_LAUNCH(k_lidar_composite_rays<KK>, dim3(blocks), dim3(256), 0, s, n_alive_max, n_step, N, W, T_thresh, alive_count, \
               rays_alive, rays_t, rays, sigmas, feats, deltas, xyzs, rays_o, rays_d, weights_sum, depth, image, transmittance)
    if (K == 1) LNH_INFER_COMPOSITE(1); else if (K == 2) LNH_INFER_COMPOSITE(2); else LNH_INFER_COMPOSITE(3);
#undef LNH_INFER_COMPOSITE
    return lnh_check_launch("lnh_lidar_composite_rays");
}

int lnh_alive_compact(uint32_t n_alive_max, const int32_t *alive_count, const int32_t *rays_alive, int32_t *rays_alive_out,
                      int32_t *alive_count_out, lnh_stream_t stream) {
    LNH_REQUIRE(alive_count && rays_alive && rays_alive_out && alive_count_out, LNH_ERR_INVALID_ARG,
                "alive_compact: null pointer");
    LNH_REQUIRE(rays_alive != rays_alive_out && alive_count != alive_count_out, LNH_ERR_INVALID_ARG,
                "alive_compact: the list and its count are compacted into the OTHER half of the ping-pong pair");
    LNH_LAUNCH(k_alive_compact, dim3(1), dim3(1024), 0, (hipStream_t)stream, n_alive_max, alive_count, rays_alive,
               rays_alive_out, alive_count_out);
    return lnh_check_launch("lnh_alive_compact");
}

}  // extern "C"
