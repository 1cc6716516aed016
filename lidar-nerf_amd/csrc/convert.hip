// convert.hip — LiDAR point cloud <-> range image ("pano") on the GPU: the step before (data preparation) and after
// (point-cloud export) the training path.  Semantics: lidarnerf/convert.py:99-160 (lidar_to_pano_with_intensities) and
// 194-237 (pano_to_lidar_with_intensities), which run as per-point Python loops / NumPy broadcasts on the host.
//
// lidar -> pano: the reference walks the points in order and keeps, per pixel, the nearest point (strict '>' — the
// first of equally near points wins).  Here every point does one 64-bit atomicMin on its pixel with the key
// (float bits of dist << 32 | point index): distances are positive, so their bit patterns order like the floats, and
// the index breaks ties towards the earlier point.  A second pass resolves keys into (dist, intensity).
// Arithmetic follows the reference's float32 NumPy scalars (angles in fp32, constants rounded to fp32 where NumPy's
// weak-scalar promotion rounds them); atan2 is evaluated in double and rounded to float, which reproduces a
// correctly-rounded atan2f.
//
// The bbox-mask variant (convert.py:4-97) is the same key pass with a resolve that applies the box window; the z-buffer
// ("fpa") variant (convert.py:253-361) keeps the z_buffer_len nearest points per pixel and is a count / scan / scatter /
// resolve pipeline further down.  All three project with pano_pixel().
#include "common.h"
#include "pano_geom.h"
#include "scan.h"

namespace {

// Point -> pixel, shared by the closest-point, bbox-mask and z-buffer paths (pano_geom.h: the one copy of the arithmetic).
__device__ __forceinline__ uint32_t pano_pixel(const float *__restrict__ pts, uint32_t i, const PanoGeom &g, float &dist) {
    return pano_pixel_xyz<false>(pts[(size_t)i * 4], pts[(size_t)i * 4 + 1], pts[(size_t)i * 4 + 2], g, dist);
}
__device__ __forceinline__ unsigned long long pano_key(float dist, uint32_t i) {
    return ((unsigned long long)__float_as_uint(dist) << 32) | i;
}

__global__ void __launch_bounds__(256)
k_lidar_to_pano_keys(const float *__restrict__ pts, uint32_t N, PanoGeom g, unsigned long long *__restrict__ keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float dist;
    const uint32_t p = pano_pixel(pts, i, g, dist);
    if (p == kNoPixel) return;
    atomicMin(&keys[p], pano_key(dist, i));
}

__global__ void __launch_bounds__(256)
k_lidar_to_pano_resolve(const float *__restrict__ pts, const unsigned long long *__restrict__ keys, uint32_t HW,
                        float *__restrict__ pano, float *__restrict__ intens) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const unsigned long long k = keys[p];
    const bool hit = k != ~0ull;
    pano[p] = hit ? __uint_as_float((uint32_t)(k >> 32)) : 0.0f;
    intens[p] = hit ? pts[(size_t)(uint32_t)k * 4 + 3] : 0.0f;
}

// bbox-mask variant (convert.py:4-97): the closest point inside the window rows [r0,r1) x columns [c0,c1), intensity divided
// by max_intensity in float32; outside the window pano = -1, intensity = 0 (the reference never writes a point there).
__global__ void __launch_bounds__(256)
k_lidar_to_pano_resolve_masked(const float *__restrict__ pts, const unsigned long long *__restrict__ keys, uint32_t HW,
                               uint32_t W, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, float max_intensity,
                               float *__restrict__ pano, float *__restrict__ intens) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const uint32_t r = p / W, c = p % W;
    const bool inside = r >= r0 && r < r1 && c >= c0 && c < c1;
    const unsigned long long k = keys[p];
    const bool hit = inside && k != ~0ull;
    pano[p] = hit ? __uint_as_float((uint32_t)(k >> 32)) : (inside ? 0.0f : -1.0f);
    intens[p] = hit ? pts[(size_t)(uint32_t)k * 4 + 3] / max_intensity : 0.0f;
}

// ------------------------------------------------------------------------------------------- z-buffer ("fpa") variant
// convert.py:253-361 (lidar_to_pano_with_intensities_fpa + parse_z_buffer).  Four launches on one stream; the launch
// boundaries are the only ordering there is, and the only atomics are integer ones:
//   k_fpa_count    one thread per point: pix[i] = pixel id (kNoPixel = dropped), count[pixel] += 1
//   k_fpa_scan     ONE workgroup: offset = exclusive scan of count (scan.h workgroup_scan)
//   k_fpa_scatter  one thread per point: keys[offset[pixel] + cursor[pixel]++] = (dist bits << 32 | point index)
//   k_fpa_resolve  one wavefront per pixel: the reference's rule on the bucket, read as a SET (slot order is arbitrary)
// Workspace: keys u64[N] | pix u32[N] | count u32[HW] | cursor u32[HW] | offset u32[HW].
__global__ void __launch_bounds__(256)
k_fpa_count(const float *__restrict__ pts, uint32_t N, PanoGeom g, uint32_t *__restrict__ pix,
            uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float dist;
    const uint32_t p = pano_pixel(pts, i, g, dist);
    pix[i] = p;
    if (p != kNoPixel) atomicAdd(&count[p], 1u);
}

__global__ void __launch_bounds__(kScanThreads)
k_fpa_scan(const uint32_t *__restrict__ count, uint32_t *__restrict__ offset, uint32_t HW) {
    (void)workgroup_scan<uint32_t>(
        HW, 0u, [&](uint32_t p, bool) { return count[p]; }, [&](uint32_t p, uint32_t off) { offset[p] = off; });
}

__global__ void __launch_bounds__(256)
k_fpa_scatter(const float *__restrict__ pts, uint32_t N, const uint32_t *__restrict__ pix,
              const uint32_t *__restrict__ offset, uint32_t *__restrict__ cursor, unsigned long long *__restrict__ keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t p = pix[i];
    if (p == kNoPixel) return;
    const float x = pts[(size_t)i * 4], y = pts[(size_t)i * 4 + 1], z = pts[(size_t)i * 4 + 2];
    const float dist = sqrtf(x * x + y * y + z * z);  // the value pano_pixel() tested in k_fpa_count
    keys[offset[p] + atomicAdd(&cursor[p], 1u)] = pano_key(dist, i);
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

// The reference's buffer of a pixel with n points, L = z_buffer_len: arrival (index) order while n <= L, else the L smallest
// under (dist, index); parse_z_buffer's slice [1:n] then leaves out the LAST of them.  Both cases are "the min(n, L) smallest
// under one total order, without the last": the order is (index, dist) for n <= L and (dist, index) for n > L, i.e. the key
// with its halves swapped or not.  Keys of a bucket are distinct (the index is), so "the smallest one above the previous one"
// extracts them in order whatever the slot order; lane j keeps the j-th.  Every lane then walks the kept ones through
// shuffles and does the same float64 sums in that order; lane 0 stores.
constexpr uint32_t kFpaPixelsPerGroup = 4;
__global__ void __launch_bounds__(64 * kFpaPixelsPerGroup)
k_fpa_resolve(const float *__restrict__ pts, const unsigned long long *__restrict__ keys,
              const uint32_t *__restrict__ count, const uint32_t *__restrict__ offset, uint32_t HW, uint32_t L,
              double threshold, float *__restrict__ pano, float *__restrict__ intens) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * kFpaPixelsPerGroup + (threadIdx.x >> 6);
    if (p >= HW) return;  // (wave-uniform; no barrier in this kernel)
    const uint32_t n = count[p];
    if (n == 0) {
        if (lane == 0) pano[p] = 0.0f, intens[p] = 0.0f;
        return;
    }
    const unsigned long long *__restrict__ bucket = keys + offset[p];
    const bool by_index = n <= L;
    const uint32_t m = by_index ? n : L;
    auto ordered = [by_index](unsigned long long k) { return by_index ? (k << 32) | (k >> 32) : k; };
    const unsigned long long first = lane < n ? ordered(bucket[lane]) : ~0ull;  // a bucket of <= 64 points is read once
    unsigned long long prev = 0, mine = ~0ull;  // (no key is 0: dist > 0; none is ~0: dist is finite, index < 2^32 - 1)
    for (uint32_t j = 0; j < m; j++) {
        unsigned long long cand = first > prev ? first : ~0ull;
        for (uint32_t e = lane + 64; e < n; e += 64) {
            const unsigned long long o = ordered(bucket[e]);
            if (o > prev && o < cand) cand = o;
        }
        prev = wave_min_u64(cand);
        if (lane == j) mine = prev;
    }
    const unsigned long long sel = by_index ? (mine << 32) | (mine >> 32) : mine;  // back to (dist bits, index)
    const float my_d = __uint_as_float((uint32_t)(sel >> 32));
    const float my_i = lane < m ? pts[(size_t)(uint32_t)sel * 4 + 3] : 0.0f;
    float out_d, out_i;
    if (m == 1) {  // one point, or z_buffer_len == 1: the nearest point itself
        out_d = __shfl(my_d, 0, 64);
        out_i = __shfl(my_i, 0, 64);
    } else {
        const uint32_t kept = m - 1;
        float dmin = __shfl(my_d, 0, 64);
        for (uint32_t j = 1; j < kept; j++) dmin = fminf(dmin, __shfl(my_d, (int)j, 64));
        const double limit = (double)dmin + threshold;
        double sw = 0.0, sd = 0.0, si = 0.0;
        for (uint32_t j = 0; j < kept; j++) {
            const double d = (double)__shfl(my_d, (int)j, 64), it = (double)__shfl(my_i, (int)j, 64);
            if (d <= limit) {
                const double w = 1.0 / d;
                sw += w;
                sd += d * w;
                si += it * w;
            }
        }
        out_d = (float)(sd / sw);
        out_i = (float)(si / sw);
    }
    if (lane == 0) pano[p] = out_d, intens[p] = out_i;
}

// pano -> points (dense [H*W,4] + validity; the caller compacts in pixel order like np.where)
__global__ void __launch_bounds__(256)
k_pano_to_lidar(const float *__restrict__ pano, const float *__restrict__ intens, uint32_t H, uint32_t W, float fov_up,
                float fov, float *__restrict__ pts, uint8_t *__restrict__ valid) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= H * W) return;
    const uint32_t j = p / W, i = p % W;
    const float d = pano[p];
    float x, y, z;
    pano_point(j, i, H, W, fov_up, fov, d, x, y, z);  // (pano_geom.h: shared with the fused points meter)
    pts[(size_t)p * 4] = x;
    pts[(size_t)p * 4 + 1] = y;
    pts[(size_t)p * 4 + 2] = z;
    pts[(size_t)p * 4 + 3] = intens ? intens[p] : 0.0f;
    valid[p] = d != 0.0f;
}

constexpr uint64_t kFpaMaxPixels = 1ull << 24;
// byte offsets of the fpa workspace's arrays (keys first: the only 8-byte type)
struct FpaLayout {
    uint64_t keys, pix, count, cursor, offset, bytes;
};
FpaLayout fpa_layout(uint64_t N, uint64_t HW) {
    FpaLayout l;
    l.keys = 0;
    l.pix = l.keys + 8 * N;
    l.count = l.pix + 4 * N;
    l.cursor = l.count + 4 * HW;
    l.offset = l.cursor + 4 * HW;
    l.bytes = (l.offset + 4 * HW + 15) & ~15ull;
    return l;
}

}  // namespace

extern "C" {

int lnh_lidar_to_pano(const float *points, uint32_t N, uint32_t H, uint32_t W, float fov_up, float fov, float max_depth,
                      void *keys_scratch, float *pano, float *intensities, lnh_stream_t stream) {
    LNH_REQUIRE((points || N == 0) && keys_scratch && pano && intensities, LNH_ERR_INVALID_ARG, "lidar_to_pano: null pointer");
    LNH_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W < 0xffffffffull, LNH_ERR_INVALID_ARG, "lidar_to_pano: bad image size");
    LNH_REQUIRE(fov > 0.0f, LNH_ERR_INVALID_ARG, "lidar_to_pano: fov must be positive");
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    LNH_REQUIRE(hipMemsetAsync(keys_scratch, 0xff, (size_t)H * W * 8, s) == hipSuccess, LNH_ERR_LAUNCH,
                "lidar_to_pano: hipMemsetAsync failed");
    const PanoGeom g = pano_geom(H, W, fov_up, fov, max_depth);
    if (N) {
        LNH_LAUNCH(k_lidar_to_pano_keys, dim3(div_up(N, 256)), dim3(256), 0, s, points, N, g,
                   (unsigned long long *)keys_scratch);
        int rc = lnh_check_launch("lnh_lidar_to_pano(keys)");
        if (rc) return rc;
    }
    LNH_LAUNCH(k_lidar_to_pano_resolve, dim3(div_up(H * W, 256)), dim3(256), 0, s, points,
               (const unsigned long long *)keys_scratch, H * W, pano, intensities);
    return lnh_check_launch("lnh_lidar_to_pano(resolve)");
}

int lnh_lidar_to_pano_masked(const float *points, uint32_t N, uint32_t H, uint32_t W, float fov_up, float fov,
                             float max_depth, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, float max_intensity,
                             void *keys_scratch, float *pano, float *intensities, lnh_stream_t stream) {
    LNH_REQUIRE((points || N == 0) && keys_scratch && pano && intensities, LNH_ERR_INVALID_ARG,
                "lidar_to_pano_masked: null pointer");
    LNH_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W < 0xffffffffull, LNH_ERR_INVALID_ARG,
                "lidar_to_pano_masked: bad image size");
    LNH_REQUIRE(fov > 0.0f, LNH_ERR_INVALID_ARG, "lidar_to_pano_masked: fov must be positive");
    LNH_REQUIRE(r0 <= r1 && r1 <= H && c0 <= c1 && c1 <= W, LNH_ERR_INVALID_ARG,
                "lidar_to_pano_masked: window [%u,%u) x [%u,%u) is not inside the %u x %u image", r0, r1, c0, c1, H, W);
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    LNH_REQUIRE(hipMemsetAsync(keys_scratch, 0xff, (size_t)H * W * 8, s) == hipSuccess, LNH_ERR_LAUNCH,
                "lidar_to_pano_masked: hipMemsetAsync failed");
    const PanoGeom g = pano_geom(H, W, fov_up, fov, max_depth);
    if (N) {
        LNH_LAUNCH(k_lidar_to_pano_keys, dim3(div_up(N, 256)), dim3(256), 0, s, points, N, g,
                   (unsigned long long *)keys_scratch);
        int rc = lnh_check_launch("lnh_lidar_to_pano_masked(keys)");
        if (rc) return rc;
    }
    LNH_LAUNCH(k_lidar_to_pano_resolve_masked, dim3(div_up(H * W, 256)), dim3(256), 0, s, points,
               (const unsigned long long *)keys_scratch, H * W, W, r0, r1, c0, c1, max_intensity, pano, intensities);
    return lnh_check_launch("lnh_lidar_to_pano_masked(resolve)");
}

uint64_t lnh_lidar_to_pano_fpa_workspace_size(uint64_t N, uint32_t H, uint32_t W) {
    const uint64_t HW = (uint64_t)H * W;
    if (H < 1 || W < 1 || HW > kFpaMaxPixels || N >= (1ull << 32)) return 0;
    return fpa_layout(N, HW).bytes;
}

int lnh_lidar_to_pano_fpa(const float *points, uint64_t N, uint32_t H, uint32_t W, float fov_up, float fov,
                          float max_depth, uint32_t z_buffer_len, double threshold, void *workspace,
                          uint64_t workspace_bytes, float *pano, float *intensities, lnh_stream_t stream) {
    LNH_REQUIRE((points || N == 0) && pano && intensities, LNH_ERR_INVALID_ARG, "lidar_to_pano_fpa: null pointer");
    LNH_REQUIRE(H >= 1 && W >= 1, LNH_ERR_INVALID_ARG, "lidar_to_pano_fpa: bad image size");
    const uint64_t HW = (uint64_t)H * W;
    LNH_REQUIRE(HW <= kFpaMaxPixels, LNH_ERR_UNSUPPORTED, "lidar_to_pano_fpa: H * W = %llu, at most 2^24 pixels",
                (unsigned long long)HW);
    LNH_REQUIRE(N < (1ull << 32), LNH_ERR_UNSUPPORTED, "lidar_to_pano_fpa: N = %llu, point indices are 32 bits wide",
                (unsigned long long)N);
    LNH_REQUIRE(z_buffer_len >= 1 && z_buffer_len <= 32, LNH_ERR_UNSUPPORTED,
                "lidar_to_pano_fpa: z_buffer_len = %u, supported 1..32", z_buffer_len);
    LNH_REQUIRE(fov > 0.0f, LNH_ERR_INVALID_ARG, "lidar_to_pano_fpa: fov must be positive");
    LNH_REQUIRE(threshold >= 0.0, LNH_ERR_INVALID_ARG, "lidar_to_pano_fpa: threshold must not be negative");
    const FpaLayout l = fpa_layout(N, HW);
    LNH_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= l.bytes, LNH_ERR_INVALID_ARG,
                "lidar_to_pano_fpa: workspace of %llu bytes (8-byte aligned) needed, got %llu",
                (unsigned long long)l.bytes, (unsigned long long)workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned long long *keys = (unsigned long long *)(ws + l.keys);
    uint32_t *pix = (uint32_t *)(ws + l.pix), *count = (uint32_t *)(ws + l.count);
    uint32_t *cursor = (uint32_t *)(ws + l.cursor), *offset = (uint32_t *)(ws + l.offset);
    int rc = lnh_zero_async(count, 8 * HW, s, "lnh_lidar_to_pano_fpa(clear)");  // count and cursor are neighbours
    if (rc) return rc;
    const PanoGeom g = pano_geom(H, W, fov_up, fov, max_depth);
    const uint32_t n = (uint32_t)N, hw = (uint32_t)HW;
    if (n) {
        LNH_LAUNCH(k_fpa_count, dim3(div_up(n, 256)), dim3(256), 0, s, points, n, g, pix, count);
        if ((rc = lnh_check_launch("lnh_lidar_to_pano_fpa(count)"))) return rc;
        LNH_LAUNCH(k_fpa_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t *)count, offset, hw);
        if ((rc = lnh_check_launch("lnh_lidar_to_pano_fpa(scan)"))) return rc;
        LNH_LAUNCH(k_fpa_scatter, dim3(div_up(n, 256)), dim3(256), 0, s, points, n, (const uint32_t *)pix,
                   (const uint32_t *)offset, cursor, keys);
        if ((rc = lnh_check_launch("lnh_lidar_to_pano_fpa(scatter)"))) return rc;
    }
    // (N == 0: every count is 0 and the resolve pass reads nothing else)
    LNH_LAUNCH(k_fpa_resolve, dim3(div_up(hw, kFpaPixelsPerGroup)), dim3(64 * kFpaPixelsPerGroup), 0, s, points,
               (const unsigned long long *)keys, (const uint32_t *)count, (const uint32_t *)offset, hw, z_buffer_len,
               threshold, pano, intensities);
    return lnh_check_launch("lnh_lidar_to_pano_fpa(resolve)");
}

int lnh_pano_to_lidar(const float *pano, const float *intensities, uint32_t H, uint32_t W, float fov_up, float fov,
                      float *points, uint8_t *valid, lnh_stream_t stream) {
    LNH_REQUIRE(pano && points && valid, LNH_ERR_INVALID_ARG, "pano_to_lidar: null pointer");
    LNH_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W < 0xffffffffull, LNH_ERR_INVALID_ARG, "pano_to_lidar: bad image size");
    LNH_LAUNCH(k_pano_to_lidar, dim3(div_up(H * W, 256)), dim3(256), 0, (hipStream_t)stream, pano, intensities, H, W,
               fov_up, fov, points, valid);
    return lnh_check_launch("lnh_pano_to_lidar");
}

}  // extern "C"
