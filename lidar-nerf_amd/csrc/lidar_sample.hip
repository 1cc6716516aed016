// lidar_sample.hip — training batches drawn on the device, straight from a preloaded sequence (poses [F,4,4], range images
// [F,H,W,3]): what the reference does on the host in KITTI360Dataset.collate / NeRFMVLDataset.collate + get_lidar_rays
// (lidarnerf/dataset/base_dataset.py:16-105, kitti360_dataset.py:123-159) — frame of the step, random patch corners, pixel
// indices, ray directions, the rotation into the world frame, the gather of the targets — as ONE launch of one thread per
// ray, followed by a one-thread launch that moves the cursor on.
//
// Nothing the draw depends on is a kernel argument that changes from step to step: the frame comes from perm[cursor[0] % F]
// and the random stream from cursor[1], both read from device memory, so a launch captured in a hipGraph draws a fresh batch
// on every replay.  The cursor is advanced by a SEPARATE launch: inside the draw kernel the increment would race with the
// workgroups that have not read it yet.
//
// Random numbers: Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain C++, key
// (seed_lo, seed_hi), counter (patch or ray index, draw_lo, draw_hi, stream_id): every patch of every draw of every stream
// has its own 128-bit block, no state is carried, no atomics.  Word 0 -> row (or the flat pixel), word 1 -> column; a word r
// goes to [0, m) as (uint64(r) * m) >> 32.  tests/sampler_ref.py restates all of it in NumPy.
#include "common.h"
#include "pano_geom.h"

namespace {

struct Philox4 {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                          uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ uint32_t to_range(uint32_t r, uint32_t m) { return (uint32_t)(((uint64_t)r * m) >> 32); }

struct SampleGeom {
    uint32_t F, H, W;
    float fov_up, fov;
};

// direction of pixel (row, col) in the world frame of `pose` (row-major 4x4): R * d_local, d_local as get_lidar_rays forms it
// (base_dataset.py:72-87) — pano_geom.h's back-projection at depth 1 (x * 1.0f is x)
__device__ __forceinline__ void pixel_ray(const float *__restrict__ pose, uint32_t row, uint32_t col, const SampleGeom &g,
                                          float *__restrict__ o, float *__restrict__ d) {
    float x, y, z;
    pano_point(row, col, g.H, g.W, g.fov_up, g.fov, 1.0f, x, y, z);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d[k] = fmaf(pose[4 * k + 2], z, fmaf(pose[4 * k + 1], y, pose[4 * k] * x));
        o[k] = pose[4 * k + 3];
    }
}

template <typename T>  // T: the 32- or 16-bit word an image value is copied as (bit for bit)
__global__ void __launch_bounds__(256)
k_lidar_sample_batch(const float *__restrict__ poses, const T *__restrict__ images, SampleGeom g,
                     const int32_t *__restrict__ perm, const uint64_t *__restrict__ cursor, uint32_t seed_lo, uint32_t seed_hi,
                     uint32_t stream_id, uint32_t n, uint32_t px, uint32_t py, int32_t frame, float *__restrict__ rays_o,
                     float *__restrict__ rays_d, T *__restrict__ gt, int32_t *__restrict__ inds) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint64_t draw = cursor[1];
    // (a perm entry is taken modulo F: whatever the caller left in that buffer, no read leaves the sequence)
    const uint32_t f = frame >= 0 ? (uint32_t)frame : (uint32_t)perm[cursor[0] % g.F] % g.F;
    uint32_t row, col;
    if (px > 0) {
        const uint32_t pp = px * py, patch = r / pp, k = r % pp;
        const Philox4 x = philox4x32_10(patch, (uint32_t)draw, (uint32_t)(draw >> 32), stream_id, seed_lo, seed_hi);
        row = to_range(x.w[0], g.H - px) + k / py;  // corners in [0, H - px) x [0, W - py): base_dataset.py:55-56
        col = to_range(x.w[1], g.W - py) + k % py;
    } else {
        const Philox4 x = philox4x32_10(r, (uint32_t)draw, (uint32_t)(draw >> 32), stream_id, seed_lo, seed_hi);
        const uint32_t flat = to_range(x.w[0], g.H * g.W);
        row = flat / g.W;
        col = flat % g.W;
    }
    const uint32_t pix = row * g.W + col;
    float o[3], d[3];
    pixel_ray(poses + (size_t)f * 16, row, col, g, o, d);
    const T *src = images + ((size_t)f * g.H * g.W + pix) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        rays_o[(size_t)r * 3 + k] = o[k];
        rays_d[(size_t)r * 3 + k] = d[k];
        gt[(size_t)r * 3 + k] = src[k];
    }
    inds[r] = (int32_t)pix;
}

// after the draw (stream order): the step within the epoch and the global draw count, both + 1
__global__ void k_lidar_sample_advance(uint64_t *__restrict__ cursor) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t step = cursor[0], draws = cursor[1];
        cursor[0] = step + 1;
        cursor[1] = draws + 1;
    }
}

__global__ void __launch_bounds__(256)
k_lidar_frame_rays(const float *__restrict__ pose, SampleGeom g, float *__restrict__ rays_o, float *__restrict__ rays_d) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.H * g.W) return;
    float o[3], d[3];
    pixel_ray(pose, p / g.W, p % g.W, g, o, d);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        rays_o[(size_t)p * 3 + k] = o[k];
        rays_d[(size_t)p * 3 + k] = d[k];
    }
}

int check_geometry(const char *who, const float *poses, int32_t F, uint32_t H, uint32_t W) {
    LNH_REQUIRE(poses, LNH_ERR_INVALID_ARG, "%s: poses is null", who);
    LNH_REQUIRE(F > 0, LNH_ERR_INVALID_ARG, "%s: F must be positive (got %d)", who, F);
    LNH_REQUIRE(H >= 1 && W >= 1, LNH_ERR_INVALID_ARG, "%s: H and W must be positive (got %u x %u)", who, H, W);
    LNH_REQUIRE((uint64_t)H * W <= (1ull << 24), LNH_ERR_UNSUPPORTED,
                "%s: H * W = %llu exceeds 2^24 pixels (a pixel index must be exact in fp32)", who,
                (unsigned long long)H * W);
    return LNH_OK;
}

}  // namespace

extern "C" {

int lnh_lidar_sample_batch(const float *poses, const void *images, int image_dtype, int32_t F, uint32_t H, uint32_t W,
                           float fov_up, float fov, const int32_t *perm, uint64_t *cursor, uint32_t seed_lo,
                           uint32_t seed_hi, int32_t stream_id, int32_t n_rays, int32_t px, int32_t py, int32_t frame,
                           float *rays_o, float *rays_d, void *gt, int32_t *inds, lnh_stream_t stream) {
    const char *who = "lidar_sample_batch";
    int rc = check_geometry(who, poses, F, H, W);
    if (rc) return rc;
    LNH_REQUIRE(images, LNH_ERR_INVALID_ARG, "%s: images is null", who);
    LNH_REQUIRE(image_dtype == LNH_F32 || image_dtype == LNH_F16, LNH_ERR_UNSUPPORTED,
                "%s: image_dtype must be LNH_F32 or LNH_F16 (got %d)", who, image_dtype);
    LNH_REQUIRE(cursor, LNH_ERR_INVALID_ARG, "%s: cursor is null", who);
    LNH_REQUIRE(n_rays > 0, LNH_ERR_INVALID_ARG, "%s: n_rays must be positive (got %d)", who, n_rays);
    LNH_REQUIRE(stream_id >= 0, LNH_ERR_INVALID_ARG, "%s: stream_id must not be negative (got %d)", who, stream_id);
    if (px > 0) {
        LNH_REQUIRE(py > 0, LNH_ERR_INVALID_ARG, "%s: py must be positive when px > 0 (got px %d, py %d)", who, px, py);
        // the reference draws corners with randint(0, H - px) / randint(0, W - py), which raises on an empty range
        LNH_REQUIRE((uint32_t)px < H, LNH_ERR_INVALID_ARG, "%s: px must be smaller than H (got px %d, H %u)", who, px, H);
        LNH_REQUIRE((uint32_t)py < W, LNH_ERR_INVALID_ARG, "%s: py must be smaller than W (got py %d, W %u)", who, py, W);
    }
    LNH_REQUIRE(frame >= -1 && frame < F, LNH_ERR_INVALID_ARG, "%s: frame must be -1 or in [0, F) (got %d, F %d)", who,
                frame, F);
    LNH_REQUIRE(frame >= 0 || perm, LNH_ERR_INVALID_ARG, "%s: perm is null (needed with frame = -1)", who);
    LNH_REQUIRE(rays_o, LNH_ERR_INVALID_ARG, "%s: rays_o is null", who);
    LNH_REQUIRE(rays_d, LNH_ERR_INVALID_ARG, "%s: rays_d is null", who);
    LNH_REQUIRE(gt, LNH_ERR_INVALID_ARG, "%s: gt is null", who);
    LNH_REQUIRE(inds, LNH_ERR_INVALID_ARG, "%s: inds is null", who);
    // rows: base_dataset.py:45-52 — N = min(N, H * W), whole patches only
    const uint32_t hw = H * W, cap = (uint32_t)n_rays < hw ? (uint32_t)n_rays : hw;
    const uint32_t upx = px > 0 ? (uint32_t)px : 0u, upy = px > 0 ? (uint32_t)py : 0u;
    const uint32_t n = px > 0 ? cap / (upx * upy) * (upx * upy) : cap;
    const SampleGeom g = {(uint32_t)F, H, W, fov_up, fov};
    hipStream_t s = (hipStream_t)stream;
    if (n) {
        if (image_dtype == LNH_F16)
            LNH_LAUNCH(k_lidar_sample_batch<uint16_t>, dim3(div_up(n, 256)), dim3(256), 0, s, poses,
                       (const uint16_t *)images, g, perm, (const uint64_t *)cursor, seed_lo, seed_hi, (uint32_t)stream_id, n,
                       upx, upy, frame, rays_o, rays_d, (uint16_t *)gt, inds);
        else
            LNH_LAUNCH(k_lidar_sample_batch<uint32_t>, dim3(div_up(n, 256)), dim3(256), 0, s, poses,
                       (const uint32_t *)images, g, perm, (const uint64_t *)cursor, seed_lo, seed_hi, (uint32_t)stream_id, n,
                       upx, upy, frame, rays_o, rays_d, (uint32_t *)gt, inds);
        rc = lnh_check_launch("lnh_lidar_sample_batch(draw)");
        if (rc) return rc;
    }
    LNH_LAUNCH(k_lidar_sample_advance, dim3(1), dim3(64), 0, s, cursor);
    return lnh_check_launch("lnh_lidar_sample_batch(advance)");
}

int lnh_lidar_frame_rays(const float *poses, int32_t F, int32_t frame, uint32_t H, uint32_t W, float fov_up, float fov,
                         float *rays_o, float *rays_d, lnh_stream_t stream) {
    const char *who = "lidar_frame_rays";
    int rc = check_geometry(who, poses, F, H, W);
    if (rc) return rc;
    LNH_REQUIRE(frame >= 0 && frame < F, LNH_ERR_INVALID_ARG, "%s: frame must be in [0, F) (got %d, F %d)", who, frame, F);
    LNH_REQUIRE(rays_o, LNH_ERR_INVALID_ARG, "%s: rays_o is null", who);
    LNH_REQUIRE(rays_d, LNH_ERR_INVALID_ARG, "%s: rays_d is null", who);
    const SampleGeom g = {(uint32_t)F, H, W, fov_up, fov};
    LNH_LAUNCH(k_lidar_frame_rays, dim3(div_up((uint64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream,
               poses + (size_t)frame * 16, g, rays_o, rays_d);
    return lnh_check_launch("lnh_lidar_frame_rays");
}

}  // extern "C"
