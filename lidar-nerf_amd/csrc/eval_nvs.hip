// eval_nvs.hip — the meters of the NVS baselines' evaluation on the device: what lidarnvs/eval.py:9-135
// (eval_points_and_pano) computes from one predicted frame and its ground truth, after the NeRF-MVL crop of lidarnvs/run.py:
// 200-217, from four images to a row of numbers in an accumulator, with no host read in between.  Not the trainer's meters
// (eval_frame.hip): images are in world scale and FLATTENED first, so the SSIM is 1-D over the row-major sequence; dropped
// pixels (depth 0) take part, clamped to 1e-3; no ray-drop masking.
//
// The evaluated sequence is the pixels with mask != 0 in row-major order (every pixel with a NULL mask).  The reference
// reshapes them to their bounding rectangle, which only works when they fill it, so the sequence is addressed as that
// rectangle (nvs_ssim_tile.h) and a frame whose count differs from the rectangle's area is marked bad.
//
// Three ordinary launches per frame, ordered by the stream:
//   k_nvs_frame     one pass over the four images and the mask: per workgroup of 1024 pixels the count and the bounding
//                   rectangle of the masked pixels (integers), the three threshold counts (integers), the fp64 sums of the
//                   float32 (gt - pd)^2 and |gt_i s - pd_i s|, min / max of the clamped ground-truth depth
//   k_nvs_ssim      a workgroup owns kNvsTile positions of the 1-D SSIM: it stages their elements and the 6-element halo of both
//                   clamped images in LDS once, a thread forms S of one position in fp64; one partial sum per workgroup
//   k_nvs_finalize  one workgroup adds every partial in index order, forms the row of LNH_NVS_SLOTS doubles (chamfer and
//                   F-score copied from the LNH_PTS_* row of the same frame), stores it in the history and adds it to the
//                   accumulator
// Deterministic: integer partials are combined with integer operations, floating-point partials by fixed trees in a fixed
// order; no float atomics.  Nothing here allocates, copies or synchronises.
#include "common.h"
#include "nvs_ssim_tile.h"

namespace {

constexpr uint32_t kT = 256, kPix = 4, kBlockPix = kT * kPix;
constexpr uint32_t kMaxPixels = 1u << 24;
static_assert(kNvsTile == kT, "one SSIM position per thread");

struct NvsPart {
    double sq, ad;  // sum (gt - pd)^2, sum |gt_i s - pd_i s| of the float32 terms
    float gmin, gmax;
    uint32_t a[3];
    uint32_t n, rmin, rmax, cmin, cmax;
    uint32_t pad[2];
};
static_assert(sizeof(NvsPart) == 64, "NvsPart is one 64-byte record");

struct NvsGeom {  // the frame's integers and range from the B partials
    uint32_t n, rmin, rmax, cmin, cmax;
    float gmin, gmax;
};

__global__ void __launch_bounds__(kT)
k_nvs_frame(const float *__restrict__ gt_pano, const float *__restrict__ pd_pano, const float *__restrict__ gt_int,
            const float *__restrict__ pd_int, const uint8_t *__restrict__ mask, uint32_t W, uint32_t N, float s,
            NvsPart *__restrict__ parts) {
    __shared__ double sh[kT / 64];
    __shared__ float sh_mm[2][kT / 64];
    __shared__ uint32_t sh_u[8];  // a1, a2, a3, n, rmin, rmax, cmin, cmax
    if (threadIdx.x < 8) sh_u[threadIdx.x] = (threadIdx.x == 4 || threadIdx.x == 6) ? 0xffffffffu : 0u;
    double sq = 0.0, ad = 0.0;
    uint32_t cnt[3] = {0u, 0u, 0u}, n = 0u, rmin = 0xffffffffu, rmax = 0u, cmin = 0xffffffffu, cmax = 0u;
    float gmin = INFINITY, gmax = -INFINITY;
#pragma unroll
    for (uint32_t k = 0; k < kPix; k++) {
        const uint32_t p = blockIdx.x * kBlockPix + k * kT + threadIdx.x;
        if (p >= N) continue;
        if (mask && mask[p] == 0) continue;
        const uint32_t r = p / W, c = p - r * W;
        n++;
        rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c);
        // eval.py:81-90 in float32, in its operation order
        const float G = nvs_clamp_depth(gt_pano[p]), P = nvs_clamp_depth(pd_pano[p]);
        const float th = fmaxf(G / P, P / G);
        cnt[0] += th < 1.25f ? 1u : 0u;
        cnt[1] += th < 1.5625f ? 1u : 0u;
        cnt[2] += th < 1.953125f ? 1u : 0u;
        const float d = G - P;
        sq += (double)(d * d);
        ad += (double)fabsf(gt_int[p] * s - pd_int[p] * s);  // run.py:214-215, eval.py:114
        gmin = fminf(gmin, G);
        gmax = fmaxf(gmax, G);
    }
    const double tot_sq = block_sum<kT>(sq, sh), tot_ad = block_sum<kT>(ad, sh);
    gmin = wave_min(gmin);
    gmax = wave_max(gmax);
    if ((threadIdx.x & 63) == 0) {
        sh_mm[0][threadIdx.x >> 6] = gmin;
        sh_mm[1][threadIdx.x >> 6] = gmax;
    }
    if (n) {  // (block_sum's barriers stand between the initialisation of sh_u and these)
        if (cnt[0]) atomicAdd(&sh_u[0], cnt[0]);
        if (cnt[1]) atomicAdd(&sh_u[1], cnt[1]);
        if (cnt[2]) atomicAdd(&sh_u[2], cnt[2]);
        atomicAdd(&sh_u[3], n);
        atomicMin(&sh_u[4], rmin);
        atomicMax(&sh_u[5], rmax);
        atomicMin(&sh_u[6], cmin);
        atomicMax(&sh_u[7], cmax);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        NvsPart f;
        f.sq = tot_sq;
        f.ad = tot_ad;
        f.gmin = fminf(fminf(sh_mm[0][0], sh_mm[0][1]), fminf(sh_mm[0][2], sh_mm[0][3]));
        f.gmax = fmaxf(fmaxf(sh_mm[1][0], sh_mm[1][1]), fmaxf(sh_mm[1][2], sh_mm[1][3]));
        f.a[0] = sh_u[0]; f.a[1] = sh_u[1]; f.a[2] = sh_u[2];
        f.n = sh_u[3]; f.rmin = sh_u[4]; f.rmax = sh_u[5]; f.cmin = sh_u[6]; f.cmax = sh_u[7];
        f.pad[0] = f.pad[1] = 0u;
        parts[blockIdx.x] = f;
    }
}

// the frame's count, rectangle and ground-truth range from the B partials; every thread receives them (integer operations
// and min / max: any order gives the same bits)
__device__ __forceinline__ NvsGeom frame_geom(const NvsPart *__restrict__ parts, uint32_t B, uint32_t *sh_u, float (*sh_mm)[kT / 64]) {
    __syncthreads();
    if (threadIdx.x < 5) sh_u[threadIdx.x] = (threadIdx.x == 1 || threadIdx.x == 3) ? 0xffffffffu : 0u;
    __syncthreads();
    uint32_t n = 0u, rmin = 0xffffffffu, rmax = 0u, cmin = 0xffffffffu, cmax = 0u;
    float gmin = INFINITY, gmax = -INFINITY;
    for (uint32_t i = threadIdx.x; i < B; i += kT) {
        const NvsPart f = parts[i];
        if (!f.n) continue;
        n += f.n;
        rmin = min(rmin, f.rmin); rmax = max(rmax, f.rmax); cmin = min(cmin, f.cmin); cmax = max(cmax, f.cmax);
        gmin = fminf(gmin, f.gmin);
        gmax = fmaxf(gmax, f.gmax);
    }
    gmin = wave_min(gmin);
    gmax = wave_max(gmax);
    if ((threadIdx.x & 63) == 0) {
        sh_mm[0][threadIdx.x >> 6] = gmin;
        sh_mm[1][threadIdx.x >> 6] = gmax;
    }
    if (n) {
        atomicAdd(&sh_u[0], n);
        atomicMin(&sh_u[1], rmin);
        atomicMax(&sh_u[2], rmax);
        atomicMin(&sh_u[3], cmin);
        atomicMax(&sh_u[4], cmax);
    }
    __syncthreads();
    NvsGeom g;
    g.n = sh_u[0]; g.rmin = sh_u[1]; g.rmax = sh_u[2]; g.cmin = sh_u[3]; g.cmax = sh_u[4];
    g.gmin = fminf(fminf(sh_mm[0][0], sh_mm[0][1]), fminf(sh_mm[0][2], sh_mm[0][3]));
    g.gmax = fmaxf(fmaxf(sh_mm[1][0], sh_mm[1][1]), fmaxf(sh_mm[1][2], sh_mm[1][3]));
    return g;
}

// the sequence of a frame: its bounding rectangle, row-major (n = 0 for an empty mask).  h <= H and w <= W by construction,
// so every element's pixel lies inside the image whether or not the masked pixels fill the rectangle.
__device__ __forceinline__ NvsSeq frame_seq(const NvsGeom &g, uint32_t W) {
    NvsSeq s;
    s.r0 = g.n ? g.rmin : 0u;
    s.c0 = g.n ? g.cmin : 0u;
    s.h = g.n ? g.rmax - g.rmin + 1u : 0u;
    s.w = g.n ? g.cmax - g.cmin + 1u : 0u;
    s.W = W;
    s.n = s.h * s.w;
    return s;
}

__global__ void __launch_bounds__(kT)
k_nvs_ssim(const float *__restrict__ gt_pano, const float *__restrict__ pd_pano, uint32_t H, uint32_t W, uint32_t B,
           const NvsPart *__restrict__ parts, double *__restrict__ ssim_parts) {
    __shared__ uint32_t sh_u[5];
    __shared__ float sh_mm[2][kT / 64];
    __shared__ double sh[kT / 64];
    __shared__ float sx[kNvsStage], sy[kNvsStage];
    const NvsGeom g = frame_geom(parts, B, sh_u, sh_mm);
    const NvsSeq seq = frame_seq(g, W);
    const uint32_t staged = nvs_tile_staged(seq.n, blockIdx.x), owned = nvs_tile_positions(seq.n, blockIdx.x);
    // partials that lnh_nvs_eval_frame did not write for this H x W (a workspace of something else) must not become addresses
    const bool sane = g.n == 0u || (g.rmin <= g.rmax && g.rmax < H && g.cmin <= g.cmax && g.cmax < W);
    if (owned == 0u || !sane) {  // (uniform over the workgroup)
        if (threadIdx.x == 0) ssim_parts[blockIdx.x] = sane ? 0.0 : (double)NAN;
        return;
    }
    const uint32_t first = blockIdx.x * kNvsTile;
    for (uint32_t e = threadIdx.x; e < staged; e += kT) {  // (staged <= kNvsStage, first + e < n)
        const uint32_t p = nvs_seq_pixel(seq, first + e);
        sx[e] = nvs_clamp_depth(gt_pano[p]);
        sy[e] = nvs_clamp_depth(pd_pano[p]);
    }
    __syncthreads();
    double c1, c2;
    nvs_ssim_constants(g.gmin, g.gmax, c1, c2);
    // structural_similarity(gt_depths, pd_depths, ...): x is the ground truth (eval.py:92-96)
    const double S = threadIdx.x < owned ? nvs_ssim_at(sx + threadIdx.x, sy + threadIdx.x, c1, c2) : 0.0;
    const double total = block_sum<kT>(S, sh);
    if (threadIdx.x == 0) ssim_parts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kT)
k_nvs_finalize(uint32_t W, uint32_t B, uint32_t SB, const NvsPart *__restrict__ parts, const double *__restrict__ ssim_parts,
               const double *__restrict__ points_row, double *__restrict__ acc, double *__restrict__ history,
               uint32_t max_frames) {
    __shared__ uint32_t sh_u[5];
    __shared__ float sh_mm[2][kT / 64];
    __shared__ double sh[kT / 64];
    __shared__ uint32_t sh_a[3];
    const NvsGeom g = frame_geom(parts, B, sh_u, sh_mm);
    const NvsSeq seq = frame_seq(g, W);
    if (threadIdx.x < 3) sh_a[threadIdx.x] = 0u;
    double sq = 0.0, ad = 0.0, ss = 0.0;
    uint32_t a[3] = {0u, 0u, 0u};
    for (uint32_t i = threadIdx.x; i < B; i += kT) {
        sq += parts[i].sq;
        ad += parts[i].ad;
        a[0] += parts[i].a[0]; a[1] += parts[i].a[1]; a[2] += parts[i].a[2];
    }
    const uint32_t used = nvs_tiles(seq.n) < SB ? nvs_tiles(seq.n) : SB;  // tiles behind the sequence wrote 0
    for (uint32_t i = threadIdx.x; i < used; i += kT) ss += ssim_parts[i];
    sq = block_sum<kT>(sq, sh);
    ad = block_sum<kT>(ad, sh);
    ss = block_sum<kT>(ss, sh);
#pragma unroll
    for (int q = 0; q < 3; q++)
        if (a[q]) atomicAdd(&sh_a[q], a[q]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = (double)g.n;
    double row[LNH_NVS_SLOTS];
    row[LNH_NVS_DEPTH_RMSE] = sqrt(sq / n);
    row[LNH_NVS_DEPTH_A1] = (double)sh_a[0] / n;
    row[LNH_NVS_DEPTH_A2] = (double)sh_a[1] / n;
    row[LNH_NVS_DEPTH_A3] = (double)sh_a[2] / n;
    row[LNH_NVS_DEPTH_SSIM] = seq.n >= kNvsWin ? ss / (double)nvs_positions(seq.n) : (double)NAN;
    row[LNH_NVS_INTENSITY_MAE] = ad / n;
    row[LNH_NVS_CHAMFER] = points_row[LNH_PTS_CHAMFER];
    row[LNH_NVS_FSCORE] = points_row[LNH_PTS_FSCORE];
    row[LNH_NVS_CROP_R0] = (double)seq.r0;
    row[LNH_NVS_CROP_C0] = (double)seq.c0;
    row[LNH_NVS_CROP_H] = (double)seq.h;
    row[LNH_NVS_CROP_W] = (double)seq.w;
    row[LNH_NVS_N] = n;
    row[LNH_NVS_DATA_RANGE] = g.n ? (double)(g.gmax - g.gmin) : (double)NAN;
    row[LNH_NVS_SUM_SQ] = sq;
    row[LNH_NVS_SUM_ABS] = ad;
    row[LNH_NVS_FRAMES] = 1.0;
    // a row the means cannot use: an empty mask, fewer than 7 pixels, masked pixels that do not fill their rectangle (the
    // reference's reshape raises, run.py:212-217), a non-finite metric, or a bad points row.  It is still added — the host
    // refuses an accumulator that counts one (nvs_eval.NVSFrameEvaluator.measure)
    bool bad = g.n < kNvsWin || g.n != seq.n || points_row[LNH_PTS_BAD] != 0.0;
    for (int q = LNH_NVS_DEPTH_RMSE; q <= LNH_NVS_FSCORE; q++) bad = bad || !isfinite(row[q]);
    row[LNH_NVS_BAD] = bad ? 1.0 : 0.0;
    const double frame = acc[LNH_NVS_FRAMES];
    if (history && frame >= 0.0 && frame < (double)max_frames) {
        double *dst = history + (size_t)frame * LNH_NVS_SLOTS;
        for (int q = 0; q < LNH_NVS_SLOTS; q++) dst[q] = row[q];
    }
    for (int q = 0; q < LNH_NVS_SLOTS; q++) acc[q] += row[q];
}

struct NvsWs {
    uint32_t B, SB;
    uint64_t off_ssim, bytes;
};

bool nvs_ws(uint32_t H, uint32_t W, NvsWs &ws) {
    const uint64_t N = (uint64_t)H * W;
    if (N < 1 || N > kMaxPixels) return false;
    ws.B = div_up(N, kBlockPix);
    ws.SB = nvs_tiles((uint32_t)N) ? nvs_tiles((uint32_t)N) : 1u;
    ws.off_ssim = (uint64_t)ws.B * sizeof(NvsPart);
    ws.bytes = ws.off_ssim + (uint64_t)ws.SB * sizeof(double);
    return true;
}

int nvs_common(const char *who, uint32_t H, uint32_t W, const void *workspace, uint64_t workspace_bytes, NvsWs &ws) {
    LNH_REQUIRE(H >= 1 && W >= 1, LNH_ERR_INVALID_ARG, "%s: H (%u) and W (%u) must be at least 1", who, H, W);
    LNH_REQUIRE((uint64_t)H * W <= kMaxPixels, LNH_ERR_UNSUPPORTED, "%s: at most 2^24 pixels per frame (H %u, W %u)", who, H, W);
    nvs_ws(H, W, ws);
    LNH_REQUIRE(workspace && workspace_bytes >= ws.bytes && ((uintptr_t)workspace & 7) == 0, LNH_ERR_INVALID_ARG,
                "%s: workspace of %llu bytes, need %llu (8-byte aligned, not null)", who, (unsigned long long)workspace_bytes,
                (unsigned long long)ws.bytes);
    return LNH_OK;
}

}  // namespace

extern "C" {

uint64_t lnh_nvs_eval_workspace_bytes(uint32_t H, uint32_t W) {
    NvsWs ws;
    return nvs_ws(H, W, ws) ? ws.bytes : 0;
}

int lnh_nvs_eval_frame(const float *gt_pano, const float *pd_pano, const float *gt_int, const float *pd_int,
                       const uint8_t *mask, uint32_t H, uint32_t W, float intensity_scale, void *workspace,
                       uint64_t workspace_bytes, lnh_stream_t stream) {
    LNH_REQUIRE(gt_pano && pd_pano, LNH_ERR_INVALID_ARG, "nvs_eval_frame: null pano pointer (gt_pano, pd_pano)");
    LNH_REQUIRE(gt_int && pd_int, LNH_ERR_INVALID_ARG, "nvs_eval_frame: null intensity pointer (gt_int, pd_int)");
    LNH_REQUIRE((((uintptr_t)gt_pano | (uintptr_t)pd_pano | (uintptr_t)gt_int | (uintptr_t)pd_int) & 3) == 0, LNH_ERR_INVALID_ARG,
                "nvs_eval_frame: the images must be 4-byte aligned");
    LNH_REQUIRE(intensity_scale == intensity_scale && intensity_scale > 0.0f && intensity_scale < INFINITY, LNH_ERR_INVALID_ARG,
                "nvs_eval_frame: intensity_scale must be positive and finite (1 for KITTI-360, 255 for NeRF-MVL)");
    NvsWs ws;
    if (int rc = nvs_common("nvs_eval_frame", H, W, workspace, workspace_bytes, ws)) return rc;
    LNH_LAUNCH(k_nvs_frame, dim3(ws.B), dim3(kT), 0, (hipStream_t)stream, gt_pano, pd_pano, gt_int, pd_int, mask, W, H * W,
               intensity_scale, (NvsPart *)workspace);
    return lnh_check_launch("lnh_nvs_eval_frame");
}

int lnh_nvs_eval_ssim(const float *gt_pano, const float *pd_pano, const uint8_t *mask, uint32_t H, uint32_t W,
                      void *workspace, uint64_t workspace_bytes, lnh_stream_t stream) {
    LNH_REQUIRE(gt_pano && pd_pano, LNH_ERR_INVALID_ARG, "nvs_eval_ssim: null pano pointer (gt_pano, pd_pano)");
    LNH_REQUIRE((((uintptr_t)gt_pano | (uintptr_t)pd_pano) & 3) == 0, LNH_ERR_INVALID_ARG,
                "nvs_eval_ssim: the images must be 4-byte aligned");
    (void)mask;  // the sequence's rectangle comes from the partials lnh_nvs_eval_frame left for this mask
    NvsWs ws;
    if (int rc = nvs_common("nvs_eval_ssim", H, W, workspace, workspace_bytes, ws)) return rc;
    LNH_LAUNCH(k_nvs_ssim, dim3(ws.SB), dim3(kT), 0, (hipStream_t)stream, gt_pano, pd_pano, H, W, ws.B,
               (const NvsPart *)workspace, (double *)((char *)workspace + ws.off_ssim));
    return lnh_check_launch("lnh_nvs_eval_ssim");
}

int lnh_nvs_eval_finalize(uint32_t H, uint32_t W, const void *workspace, uint64_t workspace_bytes, const double *points_row,
                          double *accumulator, double *history, uint32_t max_frames, lnh_stream_t stream) {
    LNH_REQUIRE(points_row, LNH_ERR_INVALID_ARG,
                "nvs_eval_finalize: null points_row pointer (the LNH_PTS_* row of the same frame, on the device)");
    LNH_REQUIRE(accumulator, LNH_ERR_INVALID_ARG, "nvs_eval_finalize: null accumulator pointer");
    LNH_REQUIRE((((uintptr_t)accumulator | (uintptr_t)history | (uintptr_t)points_row) & 7) == 0, LNH_ERR_INVALID_ARG,
                "nvs_eval_finalize: points_row, accumulator and history must be 8-byte aligned");
    LNH_REQUIRE(history || max_frames == 0, LNH_ERR_INVALID_ARG, "nvs_eval_finalize: null history pointer with max_frames %u",
                max_frames);
    NvsWs ws;
    if (int rc = nvs_common("nvs_eval_finalize", H, W, workspace, workspace_bytes, ws)) return rc;
    LNH_LAUNCH(k_nvs_finalize, dim3(1), dim3(kT), 0, (hipStream_t)stream, W, ws.B, ws.SB, (const NvsPart *)workspace,
               (const double *)((const char *)workspace + ws.off_ssim), points_row, accumulator, history, max_frames);
    return lnh_check_launch("lnh_nvs_eval_finalize");
}

}  // extern "C"
