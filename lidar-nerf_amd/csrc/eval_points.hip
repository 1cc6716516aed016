// eval_points.hip — the points meter of one evaluation frame on the device: what the reference's PointsMeter (nerf/utils.py:
// 375-427) computes from the predicted and the ground-truth range image — both back-projected to point clouds, the chamfer
// distance (extern/chamfer3D) and the F-score (extern/fscore.py) between them — from two depth images to a row of numbers in
// an accumulator, with no host read in between.
//
//   k_pts_count    per workgroup of 1024 pixels: how many have a metric depth != 0, for both images
//   k_pts_write    scans those counts (every workgroup adds up its predecessors'), scans its own pixels, and writes the
//                  back-projected points (pano_geom.h) densely, in row-major pixel order, as 16-byte points; the last
//                  workgroup writes the two totals
//   k_pts_nn       both directions of the brute-force nearest-neighbour search.  A workgroup owns 1024 query points, four per
//                  lane in registers, and ONE slice of the target cloud, which it streams through LDS in 1024-point tiles;
//                  every lane reads the same 16-byte target (one broadcast ds_read_b128 per 4 x 64 pairs).  Per pair the
//                  arithmetic of k_chamfer_nn (metrics.hip), fmaf(dz, dz, fmaf(dy, dy, dx * dx)) on target - query, strict
//                  '<' in target order.  It leaves (float bits of the squared distance << 32 | target index) per query and
//                  slice: a non-negative float orders like its bits, the index breaks ties towards the earlier target
//   k_pts_resolve  integer minimum of a query's keys over the slices -> dist, idx (independent of scheduling: plain stores,
//                  no atomics)
//   k_pts_finalize one workgroup: fp64 sums of both distance arrays in a fixed order, the threshold counts, the row of
//                  LNH_PTS_SLOTS doubles into the history and onto the accumulator (the conventions of k_eval_finalize)
// Counts live in device memory; grids are sized for the capacity H * W and surplus workgroups leave at once.
#include "common.h"
#include "pano_geom.h"

namespace {

typedef float float2_t __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr uint32_t kT = 256, kPix = 4, kBlockPix = kT * kPix;
constexpr uint32_t kQ = 4, kTileQ = kT * kQ;  // query points per lane / per workgroup
constexpr uint32_t kTileT = 1024;             // target points per LDS tile (16 KiB)
constexpr uint32_t kSliceAlign = 64, kMaxSlices = 32, kTargetGroups = 1024;  // workgroups per direction the split aims at
constexpr uint32_t kMaxPixels = 1u << 24;

// metric depths as PointsMeter.update forms them (metrics.py:156 on what evaluate.py:122-126 hands over): torch divides a
// float tensor by a host scalar as a multiplication by the float32 reciprocal; the ground-truth depth is first multiplied by
// the ray-drop channel, whose -1 (outside the NeRF-MVL window) counts as -1 * 0
__device__ __forceinline__ float pred_metric(const float *pred, uint32_t p, float inv_scale) { return pred[p] * inv_scale; }
__device__ __forceinline__ float gt_metric(const float *gt, uint32_t p, int mvl, float inv_scale) {
    float gr = gt[(size_t)p * 3];
    if (mvl) gr = gr * (gr == -1.0f ? 0.0f : 1.0f);
    return gt[(size_t)p * 3 + 2] * gr * inv_scale;
}

__global__ void __launch_bounds__(kT)
k_pts_count(const float *__restrict__ pred, const float *__restrict__ gt, uint32_t N, float inv_scale, int mvl,
            uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t c0 = 0u, c1 = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPix; k++) {
        const uint32_t p = blockIdx.x * kBlockPix + threadIdx.x * kPix + k;
        if (p >= N) break;
        c0 += pred_metric(pred, p, inv_scale) != 0.0f ? 1u : 0u;
        c1 += gt_metric(gt, p, mvl, inv_scale) != 0.0f ? 1u : 0u;
    }
    if (c0) atomicAdd(&sh[0], c0);
    if (c1) atomicAdd(&sh[1], c1);
    __syncthreads();
    if (threadIdx.x < 2) block_counts[blockIdx.x * 2 + threadIdx.x] = sh[threadIdx.x];
}

__global__ void __launch_bounds__(kT)
k_pts_write(const float *__restrict__ pred, const float *__restrict__ gt, uint32_t H, uint32_t W, float fov_up, float fov,
            float inv_scale, int mvl, const uint32_t *__restrict__ block_counts, float4 *__restrict__ cloud0,
            float4 *__restrict__ cloud1, uint32_t *__restrict__ counts) {
    __shared__ uint32_t sh_base[2];
    __shared__ uint32_t sh_wave[kT / 64];
    const uint32_t N = H * W;
    if (threadIdx.x < 2) sh_base[threadIdx.x] = 0u;
    __syncthreads();
    {   // points of the workgroups before this one (integer adds: any order gives the same bits)
        uint32_t b0 = 0u, b1 = 0u;
        for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kT) {
            b0 += block_counts[b * 2];
            b1 += block_counts[b * 2 + 1];
        }
        if (b0) atomicAdd(&sh_base[0], b0);
        if (b1) atomicAdd(&sh_base[1], b1);
    }
    const uint32_t p0 = blockIdx.x * kBlockPix + threadIdx.x * kPix;
    float d0[kPix], d1[kPix];
    uint32_t packed = 0u;  // this lane's counts: cloud 0 in the low half, cloud 1 in the high half (<= 1024 per workgroup)
#pragma unroll
    for (uint32_t k = 0; k < kPix; k++) {
        const uint32_t p = p0 + k;
        d0[k] = p < N ? pred_metric(pred, p, inv_scale) : 0.0f;
        d1[k] = p < N ? gt_metric(gt, p, mvl, inv_scale) : 0.0f;
        packed += (d0[k] != 0.0f ? 1u : 0u) + (d1[k] != 0.0f ? 0x10000u : 0u);
    }
    const uint32_t incl = wave_scan_add_u32(packed);
    if ((threadIdx.x & 63) == 63) sh_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - packed, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kT / 64; w++) {
        if (w < (threadIdx.x >> 6)) before += sh_wave[w];
        total += sh_wave[w];
    }
    uint32_t o0 = sh_base[0] + (before & 0xffffu), o1 = sh_base[1] + (before >> 16);
#pragma unroll
    for (uint32_t k = 0; k < kPix; k++) {
        const uint32_t p = p0 + k;
        if (p >= N) break;
        const uint32_t j = p / W, i = p - j * W;
        float x, y, z;
        if (d0[k] != 0.0f && o0 < N) {  // (o < N always: at most one point per pixel)
            pano_point(j, i, H, W, fov_up, fov, d0[k], x, y, z);
            cloud0[o0++] = make_float4(x, y, z, 0.0f);
        }
        if (d1[k] != 0.0f && o1 < N) {
            pano_point(j, i, H, W, fov_up, fov, d1[k], x, y, z);
            cloud1[o1++] = make_float4(x, y, z, 0.0f);
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        counts[0] = sh_base[0] + (total & 0xffffu);
        counts[1] = sh_base[1] + (total >> 16);
    }
}

// target points per slice: the cloud of m points split over at most S workgroups
__device__ __forceinline__ uint32_t slice_len(uint32_t m, uint32_t S) {
    const uint32_t l = (m + S - 1) / S;
    return max((l + kSliceAlign - 1) / kSliceAlign * kSliceAlign, kSliceAlign);
}

__global__ void __launch_bounds__(kT)
k_pts_nn(const float4 *__restrict__ cloud0, const float4 *__restrict__ cloud1, const uint32_t *__restrict__ counts,
         uint32_t cap, uint32_t S, u64 *__restrict__ parts) {
    __shared__ float4 tile[kTileT];
    const uint32_t dir = blockIdx.z;
    const float4 *__restrict__ qc = dir ? cloud1 : cloud0;
    const float4 *__restrict__ tc = dir ? cloud0 : cloud1;
    const uint32_t n = min(counts[dir], cap), m = min(counts[1 - dir], cap);
    const uint32_t q0 = blockIdx.x * kTileQ;
    if (q0 >= n) return;
    const uint32_t L = slice_len(m, S), t0 = blockIdx.y * L;
    if (t0 >= m) return;
    const uint32_t t1 = min(m, t0 + L);
    float2_t qx[kQ / 2], qy[kQ / 2], qz[kQ / 2];
    float best[kQ];
    uint32_t best_i[kQ];
#pragma unroll
    for (uint32_t e = 0; e < kQ; e++) {
        const float4 q = qc[min(q0 + e * kT + threadIdx.x, n - 1)];
        qx[e / 2][e % 2] = q.x;
        qy[e / 2][e % 2] = q.y;
        qz[e / 2][e % 2] = q.z;
        best[e] = INFINITY;
        best_i[e] = t0;
    }
    for (uint32_t k0 = t0; k0 < t1; k0 += kTileT) {
        const uint32_t cnt = min(kTileT, t1 - k0);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < cnt; t += kT) tile[t] = tc[k0 + t];
        __syncthreads();
        LNH_MARK("pts_nn_pairs");
#pragma unroll 4
        for (uint32_t k = 0; k < cnt; k++) {
            const float4 p = tile[k];  // the same address in every lane: one broadcast 16-byte read
#pragma unroll
            for (uint32_t h = 0; h < kQ / 2; h++) {
                const float2_t dx = p.x - qx[h], dy = p.y - qy[h], dz = p.z - qz[h];
                // x*x + y*y + z*z as k_chamfer_nn forms it (two fused multiply-adds), two queries per instruction
                const float2_t d = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
#pragma unroll
                for (uint32_t e = 0; e < 2; e++) {
                    const bool closer = d[e] < best[h * 2 + e];
                    best[h * 2 + e] = closer ? d[e] : best[h * 2 + e];
                    best_i[h * 2 + e] = closer ? k0 + k : best_i[h * 2 + e];
                }
            }
        }
        LNH_MARK("pts_nn_pairs_end");
    }
    u64 *__restrict__ out = parts + ((size_t)dir * S + blockIdx.y) * cap;
#pragma unroll
    for (uint32_t e = 0; e < kQ; e++) {
        const uint32_t q = q0 + e * kT + threadIdx.x;
        if (q < n) out[q] = ((u64)__float_as_uint(best[e]) << 32) | best_i[e];
    }
}

__global__ void __launch_bounds__(kT)
k_pts_resolve(const uint32_t *__restrict__ counts, uint32_t cap, uint32_t S, const u64 *__restrict__ parts,
              float *__restrict__ dist0, int32_t *__restrict__ idx0, float *__restrict__ dist1, int32_t *__restrict__ idx1) {
    const uint32_t dir = blockIdx.y, q = blockIdx.x * kT + threadIdx.x;
    const uint32_t n = min(counts[dir], cap), m = min(counts[1 - dir], cap);
    if (q >= n) return;
    const uint32_t L = slice_len(m, S), used = (m + L - 1) / L;  // slices that hold a target (0 for an empty cloud)
    u64 key = ((u64)__float_as_uint(INFINITY) << 32);
    for (uint32_t s = 0; s < used; s++) key = min(key, parts[((size_t)dir * S + s) * cap + q]);
    (dir ? dist1 : dist0)[q] = __uint_as_float((uint32_t)(key >> 32));
    (dir ? idx1 : idx0)[q] = (int32_t)(uint32_t)key;
}

__global__ void __launch_bounds__(kT)
k_pts_finalize(const float *__restrict__ dist0, const float *__restrict__ dist1, const uint32_t *__restrict__ counts,
               uint32_t cap, float threshold, double *__restrict__ acc, double *__restrict__ history, uint32_t max_frames) {
    __shared__ double sh[kT / 64];
    const uint32_t n[2] = {min(counts[0], cap), min(counts[1], cap)};
    const bool empty = n[0] == 0u || n[1] == 0u;  // no nearest neighbour exists: the distance arrays are not read
    double sum[2], below[2];
    for (int c = 0; c < 2; c++) {
        const float *__restrict__ d = c ? dist1 : dist0;
        double s = 0.0, b = 0.0;
        if (!empty)
            for (uint32_t i = threadIdx.x; i < n[c]; i += kT) {
                const float v = d[i];
                s += (double)v;
                b += v < threshold ? 1.0 : 0.0;
            }
        sum[c] = block_sum<kT>(s, sh);
        below[c] = block_sum<kT>(b, sh);
    }
    if (threadIdx.x != 0) return;
    double row[LNH_PTS_SLOTS];
    const double mean0 = sum[0] / (double)n[0], mean1 = sum[1] / (double)n[1];  // (0 / 0: NaN for an empty cloud)
    const double p = below[0] / (double)n[0], r = below[1] / (double)n[1];
    const double f = 2.0 * p * r / (p + r);
    row[LNH_PTS_CHAMFER] = mean0 + mean1;
    row[LNH_PTS_FSCORE] = f != f ? 0.0 : f;  // extern/fscore.py:16: NaN (p + r == 0) counts as 0
    row[LNH_PTS_PRECISION] = p;
    row[LNH_PTS_RECALL] = r;
    row[LNH_PTS_MEAN_PRED] = mean0;
    row[LNH_PTS_MEAN_GT] = mean1;
    row[LNH_PTS_COUNT_PRED] = (double)n[0];
    row[LNH_PTS_COUNT_GT] = (double)n[1];
    row[LNH_PTS_FRAMES] = 1.0;
    // a row the means cannot use: an empty cloud (the reference averages an empty tensor), or a non-finite distance.  It is
    // still added — the host refuses an accumulator that counts one (metrics.FramePointsEvaluator.measure)
    row[LNH_PTS_BAD] = (empty || !isfinite(row[LNH_PTS_CHAMFER])) ? 1.0 : 0.0;
    const double frame = acc[LNH_PTS_FRAMES];
    if (history && frame >= 0.0 && frame < (double)max_frames) {
        double *dst = history + (size_t)frame * LNH_PTS_SLOTS;
        for (int q = 0; q < LNH_PTS_SLOTS; q++) dst[q] = row[q];
    }
    for (int q = 0; q < LNH_PTS_SLOTS; q++) acc[q] += row[q];
}

struct PtsWs {
    uint32_t B, QT, S;
    uint64_t off_parts, bytes;
};

bool pts_ws(uint64_t cap, PtsWs &ws) {
    if (cap < 1 || cap > kMaxPixels) return false;
    ws.B = div_up(cap, kBlockPix);
    ws.QT = div_up(cap, kTileQ);
    ws.S = div_up(kTargetGroups, ws.QT);
    if (ws.S > kMaxSlices) ws.S = kMaxSlices;
    ws.off_parts = ((uint64_t)ws.B * 2 * sizeof(uint32_t) + 15) / 16 * 16;
    ws.bytes = ws.off_parts + 2ull * ws.S * cap * sizeof(u64);
    return true;
}

int pts_common(const char *who, uint64_t cap, const void *workspace, uint64_t workspace_bytes, PtsWs &ws) {
    LNH_REQUIRE(cap >= 1, LNH_ERR_INVALID_ARG, "%s: H * W (the capacity of the point buffers) must be at least 1", who);
    LNH_REQUIRE(cap <= kMaxPixels, LNH_ERR_UNSUPPORTED, "%s: at most 2^24 pixels per frame (H * W = %llu)", who,
                (unsigned long long)cap);
    pts_ws(cap, ws);
    LNH_REQUIRE(workspace && workspace_bytes >= ws.bytes && ((uintptr_t)workspace & 15) == 0, LNH_ERR_INVALID_ARG,
                "%s: workspace of %llu bytes, need %llu (16-byte aligned, not null)", who, (unsigned long long)workspace_bytes,
                (unsigned long long)ws.bytes);
    return LNH_OK;
}

}  // namespace

extern "C" {

uint64_t lnh_eval_points_workspace_bytes(uint32_t H, uint32_t W) {
    PtsWs ws;
    return pts_ws((uint64_t)H * W, ws) ? ws.bytes : 0;
}

int lnh_eval_points_project(const float *pred_depth, const float *gt, uint32_t H, uint32_t W, float fov_up, float fov,
                            float scale, int32_t nerf_mvl, void *workspace, uint64_t workspace_bytes, float *cloud_pred,
                            float *cloud_gt, uint32_t *counts, lnh_stream_t stream) {
    LNH_REQUIRE(pred_depth, LNH_ERR_INVALID_ARG, "eval_points_project: null pred_depth pointer");
    LNH_REQUIRE(gt, LNH_ERR_INVALID_ARG, "eval_points_project: null gt pointer");
    LNH_REQUIRE(cloud_pred && cloud_gt, LNH_ERR_INVALID_ARG, "eval_points_project: null cloud pointer (cloud_pred, cloud_gt)");
    LNH_REQUIRE(counts, LNH_ERR_INVALID_ARG, "eval_points_project: null counts pointer");
    LNH_REQUIRE((((uintptr_t)cloud_pred | (uintptr_t)cloud_gt) & 15) == 0 && ((uintptr_t)counts & 3) == 0, LNH_ERR_INVALID_ARG,
                "eval_points_project: the clouds must be 16-byte aligned, counts 4-byte aligned");
    LNH_REQUIRE(scale > 0.0f, LNH_ERR_INVALID_ARG, "eval_points_project: scale must be positive");
    PtsWs ws;
    if (int rc = pts_common("eval_points_project", (uint64_t)H * W, workspace, workspace_bytes, ws)) return rc;
    const float inv_scale = 1.0f / scale;
    uint32_t *block_counts = (uint32_t *)workspace;
    LNH_LAUNCH(k_pts_count, dim3(ws.B), dim3(kT), 0, (hipStream_t)stream, pred_depth, gt, H * W, inv_scale, nerf_mvl ? 1 : 0,
               block_counts);
    LNH_LAUNCH(k_pts_write, dim3(ws.B), dim3(kT), 0, (hipStream_t)stream, pred_depth, gt, H, W, fov_up, fov, inv_scale,
               nerf_mvl ? 1 : 0, (const uint32_t *)block_counts, (float4 *)cloud_pred, (float4 *)cloud_gt, counts);
    return lnh_check_launch("lnh_eval_points_project");
}

int lnh_eval_points_nn(const float *cloud_pred, const float *cloud_gt, const uint32_t *counts, uint32_t capacity,
                       void *workspace, uint64_t workspace_bytes, float *dist_pred, int32_t *idx_pred, float *dist_gt,
                       int32_t *idx_gt, lnh_stream_t stream) {
    LNH_REQUIRE(cloud_pred && cloud_gt, LNH_ERR_INVALID_ARG, "eval_points_nn: null cloud pointer (cloud_pred, cloud_gt)");
    LNH_REQUIRE(counts, LNH_ERR_INVALID_ARG, "eval_points_nn: null counts pointer");
    LNH_REQUIRE(dist_pred && idx_pred && dist_gt && idx_gt, LNH_ERR_INVALID_ARG,
                "eval_points_nn: null output pointer (dist_pred, idx_pred, dist_gt, idx_gt)");
    LNH_REQUIRE((((uintptr_t)cloud_pred | (uintptr_t)cloud_gt) & 15) == 0 && ((uintptr_t)counts & 3) == 0, LNH_ERR_INVALID_ARG,
                "eval_points_nn: the clouds must be 16-byte aligned, counts 4-byte aligned");
    PtsWs ws;
    if (int rc = pts_common("eval_points_nn", capacity, workspace, workspace_bytes, ws)) return rc;
    u64 *parts = (u64 *)((char *)workspace + ws.off_parts);
    LNH_LAUNCH(k_pts_nn, dim3(ws.QT, ws.S, 2), dim3(kT), 0, (hipStream_t)stream, (const float4 *)cloud_pred,
               (const float4 *)cloud_gt, counts, capacity, ws.S, parts);
    LNH_LAUNCH(k_pts_resolve, dim3(div_up(capacity, kT), 2), dim3(kT), 0, (hipStream_t)stream, counts, capacity, ws.S,
               (const u64 *)parts, dist_pred, idx_pred, dist_gt, idx_gt);
    return lnh_check_launch("lnh_eval_points_nn");
}

int lnh_eval_points_finalize(const float *dist_pred, const float *dist_gt, const uint32_t *counts, uint32_t capacity,
                             float threshold, double *accumulator, double *history, uint32_t max_frames,
                             lnh_stream_t stream) {
    LNH_REQUIRE(dist_pred && dist_gt, LNH_ERR_INVALID_ARG, "eval_points_finalize: null distance pointer (dist_pred, dist_gt)");
    LNH_REQUIRE(counts, LNH_ERR_INVALID_ARG, "eval_points_finalize: null counts pointer");
    LNH_REQUIRE(accumulator, LNH_ERR_INVALID_ARG, "eval_points_finalize: null accumulator pointer");
    LNH_REQUIRE((((uintptr_t)accumulator | (uintptr_t)history) & 7) == 0, LNH_ERR_INVALID_ARG,
                "eval_points_finalize: accumulator and history must be 8-byte aligned");
    LNH_REQUIRE(history || max_frames == 0, LNH_ERR_INVALID_ARG, "eval_points_finalize: null history pointer with max_frames %u",
                max_frames);
    LNH_REQUIRE(capacity >= 1, LNH_ERR_INVALID_ARG,
                "eval_points_finalize: H * W (the capacity of the point buffers) must be at least 1");
    LNH_REQUIRE(capacity <= kMaxPixels, LNH_ERR_UNSUPPORTED, "eval_points_finalize: at most 2^24 pixels per frame (H * W = %u)",
                capacity);
    LNH_REQUIRE(threshold > 0.0f, LNH_ERR_INVALID_ARG, "eval_points_finalize: threshold must be positive (squared distance)");
    LNH_LAUNCH(k_pts_finalize, dim3(1), dim3(kT), 0, (hipStream_t)stream, dist_pred, dist_gt, counts, capacity, threshold,
               accumulator, history, max_frames);
    return lnh_check_launch("lnh_eval_points_finalize");
}

}  // extern "C"
