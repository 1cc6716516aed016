// eval_frame.hip — the evaluation epilogue of one LiDAR frame on the device: what the reference's Trainer.eval_step /
// test_step do after model.render (nerf/utils.py:886-1009: ray-drop masking, the NeRF-MVL valid window, the validation
// loss) and what evaluate_one_epoch's meters then compute from the returned images (1357-1366 with MAEMeter, RMSEMeter,
// DepthMeter, 226-362), with no host read between the rendered outputs and the accumulated numbers.
//
// Four ordinary launches per frame, ordered by the stream (a frame is ~68 k pixels: the work is launch-bound, and a
// dependency carried by a launch boundary needs no cross-workgroup hand-off):
//   k_eval_any       per workgroup: "some pixel predicts ray-drop > 0.5 (and is valid)", the bounding rectangle and the
//                    count of the valid pixels (ground-truth ray-drop != -1 with nerf_mvl, every pixel otherwise)
//   k_eval_frame     knows from those whether eval_step applies the mask; writes the masked images, and per workgroup the
//                    fp64 sums of the three criteria, |d intensity|, (d intensity)^2, (d depth in metres)^2, the three
//                    threshold counts and min / max of the clamped ground-truth depth
//   k_eval_ssim      mean SSIM of the clamped depth images in metres over the rectangle: a workgroup stages a 14 x 70 tile
//                    (8 x 64 windows + the 6-pixel halo) of both images in LDS once, forms the five 7-wide row sums per
//                    position, then the column sums of those — all window moments in fp64 (uxx - ux ux cancels
//                    catastrophically in fp32 at 80 m); data_range comes from k_eval_frame's partials
//   k_eval_finalize  one workgroup adds every partial in index order, forms the row of LNH_EVAL_SLOTS numbers, adds it to
//                    the accumulator and stores it in the history
// Deterministic: integer partials are combined with integer operations, floating-point partials by fixed trees in a fixed
// order; no float atomics.  Nothing here allocates, copies or synchronises.
#include "common.h"

namespace {

constexpr uint32_t kT = 256, kPix = 4, kBlockPix = kT * kPix;
constexpr uint32_t kTileR = 8, kTileC = 64, kWin = 7, kHalo = kWin - 1;
constexpr uint32_t kStageR = kTileR + kHalo, kStageC = kTileC + kHalo, kStagePitch = 72;

struct AnyPart {
    uint32_t any, rmin, rmax, cmin, cmax, nvalid, pad0, pad1;
};
struct FramePart {
    double s[6];  // criterion sums: depth, ray-drop, intensity; sum |d i| inv_scale, sum (d i)^2, sum (d depth [m])^2
    float gmin, gmax;
    uint32_t a[3];
    uint32_t pad;
};

struct EvalArgs {
    const float *image, *depth, *gt;
    uint32_t H, W, N, B;
    int32_t crit[3];
    float delta, a_r, scale, inv_i;
    int32_t mode, mvl;
};

// criterion value, reduction 'none' (the arithmetic of lnh_lidar_loss_ex's)
__device__ __forceinline__ float crit_value(int32_t c, float x, float y, float delta) {
    const float d = x - y;
    if (c == LNH_LOSS_L1) return fabsf(d);
    if (c == LNH_LOSS_MSE) return d * d;
    if (c == LNH_LOSS_HUBER) {
        const float a = fabsf(d);
        return a < delta ? 0.5f * d * d : delta * (a - 0.5f * delta);
    }
    return (1.0f - y) * x - (fminf(x, 0.0f) - log1pf(expf(-fabsf(x))));
}

// the thresholded ray-drop mask: image_lidar[:, 0] > 0.5 (utils.py:930 / 1002), in EVAL mode times the valid window (931-932)
__device__ __forceinline__ float mask_of(float pred_raydrop, bool valid, int32_t mode) {
    return (pred_raydrop > 0.5f && (valid || mode == LNH_EVAL_MODE_TEST)) ? 1.0f : 0.0f;
}

// whether intensity and depth are multiplied by the mask: eval_step `if alpha_r > 0 and not all(mask == 0)` (utils.py:936),
// test_step whenever alpha_r > 0 (1005)
__host__ __device__ __forceinline__ bool mask_applies(float alpha_r, int32_t mode, bool any) {
    return alpha_r > 0.0f && (mode == LNH_EVAL_MODE_TEST || any);
}

// numpy's in-place clamp of DepthMeter (utils.py:344-347): a NaN stays a NaN
__device__ __forceinline__ float clamp_depth(float x) { return x < 1e-3f ? 1e-3f : (x > 80.0f ? 80.0f : x); }

// combines thread-private AnyPart values of the workgroup (integer operations: any order gives the same bits)
__device__ __forceinline__ AnyPart block_any(const AnyPart &t, AnyPart *sh) {
    __syncthreads();
    if (threadIdx.x == 0) *sh = AnyPart{0u, 0xffffffffu, 0u, 0xffffffffu, 0u, 0u, 0u, 0u};
    __syncthreads();
    if (t.any) atomicOr(&sh->any, 1u);
    if (t.nvalid) {
        atomicMin(&sh->rmin, t.rmin);
        atomicMax(&sh->rmax, t.rmax);
        atomicMin(&sh->cmin, t.cmin);
        atomicMax(&sh->cmax, t.cmax);
        atomicAdd(&sh->nvalid, t.nvalid);
    }
    __syncthreads();
    return *sh;
}

__device__ __forceinline__ void any_merge(AnyPart &t, const AnyPart &p) {
    t.any |= p.any;
    if (p.nvalid) {
        t.rmin = min(t.rmin, p.rmin);
        t.rmax = max(t.rmax, p.rmax);
        t.cmin = min(t.cmin, p.cmin);
        t.cmax = max(t.cmax, p.cmax);
        t.nvalid += p.nvalid;
    }
}

// the whole frame's AnyPart from the B partials of k_eval_any
__device__ __forceinline__ AnyPart frame_any(const AnyPart *parts, uint32_t B, AnyPart *sh) {
    AnyPart t{0u, 0xffffffffu, 0u, 0xffffffffu, 0u, 0u, 0u, 0u};
    for (uint32_t i = threadIdx.x; i < B; i += blockDim.x) any_merge(t, parts[i]);
    return block_any(t, sh);
}

__global__ void __launch_bounds__(kT)
k_eval_any(EvalArgs a, AnyPart *__restrict__ parts) {
    __shared__ AnyPart sh;
    AnyPart t{0u, 0xffffffffu, 0u, 0xffffffffu, 0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kPix; k++) {
        const uint32_t p = blockIdx.x * kBlockPix + k * kT + threadIdx.x;
        if (p >= a.N) continue;
        const bool valid = !(a.mvl && a.gt[p * 3] == -1.0f);
        if (mask_of(a.image[p * 2], valid, a.mode) != 0.0f) t.any = 1u;
        if (valid) {
            const uint32_t r = p / a.W, c = p - r * a.W;
            t.rmin = min(t.rmin, r);
            t.rmax = max(t.rmax, r);
            t.cmin = min(t.cmin, c);
            t.cmax = max(t.cmax, c);
            t.nvalid++;
        }
    }
    const AnyPart tot = block_any(t, &sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = tot;
}

// test_step without a ground truth (utils.py:998-1007): the three images only
__global__ void __launch_bounds__(kT)
k_eval_mask(const float *__restrict__ image, const float *__restrict__ depth, uint32_t N, int apply,
            float *__restrict__ out_i, float *__restrict__ out_d, float *__restrict__ out_m) {
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p >= N) return;
    const float mf = mask_of(image[p * 2], true, LNH_EVAL_MODE_TEST);
    const float pi = image[p * 2 + 1], pd = depth[p];
    out_m[p] = mf;
    out_i[p] = apply ? pi * mf : pi;
    out_d[p] = apply ? pd * mf : pd;
}

__global__ void __launch_bounds__(kT)
k_eval_frame(EvalArgs a, const AnyPart *__restrict__ any_parts, FramePart *__restrict__ parts, float *__restrict__ out_i,
             float *__restrict__ out_d, float *__restrict__ out_m) {
    __shared__ AnyPart sh_any;
    __shared__ double sh[kT / 64];
    __shared__ float sh_mm[2][kT / 64];
    __shared__ uint32_t sh_a[3];
    const AnyPart tot = frame_any(any_parts, a.B, &sh_any);
    const bool apply = mask_applies(a.a_r, a.mode, tot.any != 0u);
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t cnt[3] = {0u, 0u, 0u};
    float gmin = INFINITY, gmax = -INFINITY;
#pragma unroll
    for (uint32_t k = 0; k < kPix; k++) {
        const uint32_t p = blockIdx.x * kBlockPix + k * kT + threadIdx.x;
        if (p >= a.N) continue;
        const float gr_raw = a.gt[p * 3];
        const bool valid = !(a.mvl && gr_raw == -1.0f);
        const float gr = gr_raw * (valid ? 1.0f : 0.0f);  // gt_raydrop * valid_mask (utils.py:910-911)
        const float gi = a.gt[p * 3 + 1] * gr, gd = a.gt[p * 3 + 2] * gr;
        const float pr = a.image[p * 2], pi = a.image[p * 2 + 1], pd = a.depth[p];
        const float mf = mask_of(pr, valid, a.mode);
        const float pim = apply ? pi * mf : pi, pdm = apply ? pd * mf : pd;
        out_m[p] = mf;
        out_i[p] = pim;
        out_d[p] = pdm;
        // the loss is taken over the whole frame (utils.py:940-946)
        s[0] += (double)crit_value(a.crit[0], pdm, gd, a.delta);
        s[1] += (double)crit_value(a.crit[1], pr, gr, a.delta);
        s[2] += (double)crit_value(a.crit[2], pim, gi, a.delta);
        if (!valid) continue;  // the meters see the valid window (utils.py:948-956, 1357-1366)
        s[3] += (double)fabsf(gi * a.inv_i - pim * a.inv_i);
        const float di = gi - pim;
        s[4] += (double)(di * di);
        const float P = clamp_depth(pdm / a.scale), G = clamp_depth(gd / a.scale);
        const float dd = G - P;
        s[5] += (double)(dd * dd);
        const float th = fmaxf(G / P, P / G);
        cnt[0] += th < 1.25f ? 1u : 0u;
        cnt[1] += th < 1.5625f ? 1u : 0u;
        cnt[2] += th < 1.953125f ? 1u : 0u;
        gmin = fminf(gmin, G);
        gmax = fmaxf(gmax, G);
    }
    double tot_s[6];
#pragma unroll
    for (int q = 0; q < 6; q++) tot_s[q] = block_sum<kT>(s[q], sh);
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        gmin = fminf(gmin, __shfl_xor(gmin, sft, 64));
        gmax = fmaxf(gmax, __shfl_xor(gmax, sft, 64));
    }
    __syncthreads();
    if (threadIdx.x < 3) sh_a[threadIdx.x] = 0u;
    if ((threadIdx.x & 63) == 0) {
        sh_mm[0][threadIdx.x >> 6] = gmin;
        sh_mm[1][threadIdx.x >> 6] = gmax;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; q++)
        if (cnt[q]) atomicAdd(&sh_a[q], cnt[q]);
    __syncthreads();
    if (threadIdx.x == 0) {
        FramePart f;
#pragma unroll
        for (int q = 0; q < 6; q++) f.s[q] = tot_s[q];
        f.gmin = fminf(fminf(sh_mm[0][0], sh_mm[0][1]), fminf(sh_mm[0][2], sh_mm[0][3]));
        f.gmax = fmaxf(fmaxf(sh_mm[1][0], sh_mm[1][1]), fmaxf(sh_mm[1][2], sh_mm[1][3]));
        f.a[0] = sh_a[0]; f.a[1] = sh_a[1]; f.a[2] = sh_a[2];
        f.pad = 0u;
        parts[blockIdx.x] = f;
    }
}

// min / max of the clamped ground-truth depth over the frame's partials; every thread receives them
__device__ __forceinline__ void frame_range(const FramePart *parts, uint32_t B, float (*sh)[kT / 64], float &gmin, float &gmax) {
    gmin = INFINITY;
    gmax = -INFINITY;
    for (uint32_t i = threadIdx.x; i < B; i += blockDim.x) {
        gmin = fminf(gmin, parts[i].gmin);
        gmax = fmaxf(gmax, parts[i].gmax);
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        gmin = fminf(gmin, __shfl_xor(gmin, sft, 64));
        gmax = fmaxf(gmax, __shfl_xor(gmax, sft, 64));
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = gmin;
        sh[1][threadIdx.x >> 6] = gmax;
    }
    __syncthreads();
    gmin = fminf(fminf(sh[0][0], sh[0][1]), fminf(sh[0][2], sh[0][3]));
    gmax = fmaxf(fmaxf(sh[1][0], sh[1][1]), fmaxf(sh[1][2], sh[1][3]));
}

__global__ void __launch_bounds__(kT)
k_eval_ssim(const float *__restrict__ pred_depth, const float *__restrict__ gt, uint32_t H, uint32_t W, uint32_t B,
            float scale, int mvl, const AnyPart *__restrict__ any_parts, const FramePart *__restrict__ frame_parts,
            double *__restrict__ ssim_parts) {
    __shared__ AnyPart sh_any;
    __shared__ float sh_mm[2][kT / 64];
    __shared__ double sh[kT / 64];
    __shared__ float tp[kStageR][kStagePitch], tg[kStageR][kStagePitch];
    __shared__ double rs[5][kStageR][kTileC];
    const AnyPart tot = frame_any(any_parts, B, &sh_any);
    float gmin, gmax;
    frame_range(frame_parts, B, sh_mm, gmin, gmax);
    const uint32_t part = blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t h = tot.nvalid ? tot.rmax - tot.rmin + 1 : 0u, w = tot.nvalid ? tot.cmax - tot.cmin + 1 : 0u;
    const uint32_t orow0 = blockIdx.y * kTileR, ocol0 = blockIdx.x * kTileC;
    if (h < kWin || w < kWin || orow0 >= h - kHalo || ocol0 >= w - kHalo) {  // (uniform over the workgroup)
        if (threadIdx.x == 0) ssim_parts[part] = 0.0;
        return;
    }
    const uint32_t out_h = h - kHalo, out_w = w - kHalo;
    // stage the tile and its halo: clamped depths in metres, as DepthMeter forms them (utils.py:328-329, 344-347)
    for (uint32_t e = threadIdx.x; e < kStageR * kStageC; e += kT) {
        const uint32_t r = e / kStageC, c = e - r * kStageC;
        const uint32_t rr = orow0 + r, cc = ocol0 + c;
        float P = 0.0f, G = 0.0f;
        if (rr < h && cc < w) {
            const uint32_t p = (tot.rmin + rr) * W + tot.cmin + cc;
            const float gr_raw = gt[p * 3];
            const float gr = gr_raw * ((mvl && gr_raw == -1.0f) ? 0.0f : 1.0f);
            P = clamp_depth(pred_depth[p] / scale);
            G = clamp_depth(gt[p * 3 + 2] * gr / scale);
        }
        tp[r][c] = P;
        tg[r][c] = G;
    }
    __syncthreads();
    // the five 7-wide row sums at every (row, window column) of the tile
    for (uint32_t e = threadIdx.x; e < kStageR * kTileC; e += kT) {
        const uint32_t r = e / kTileC, c = e - r * kTileC;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < kWin; j++) {
            const double x = (double)tp[r][c + j], y = (double)tg[r][c + j];
            sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
        }
        rs[0][r][c] = sx; rs[1][r][c] = sy; rs[2][r][c] = sxx; rs[3][r][c] = syy; rs[4][r][c] = sxy;
    }
    __syncthreads();
    // skimage.metrics.structural_similarity's defaults: uniform 7 x 7 window, sample covariance, K1 0.01, K2 0.03
    const double range = (double)gmax - (double)gmin;
    const double c1 = (0.01 * range) * (0.01 * range), c2 = (0.03 * range) * (0.03 * range);
    const double inv_np = 1.0 / (double)(kWin * kWin), cov_norm = (double)(kWin * kWin) / (double)(kWin * kWin - 1);
    double acc = 0.0;
    for (uint32_t e = threadIdx.x; e < kTileR * kTileC; e += kT) {
        const uint32_t r = e / kTileC, c = e - r * kTileC;
        if (orow0 + r >= out_h || ocol0 + c >= out_w) continue;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (uint32_t j = 0; j < kWin; j++)
#pragma unroll
            for (int q = 0; q < 5; q++) m[q] += rs[q][r + j][c];
        const double ux = m[0] * inv_np, uy = m[1] * inv_np, uxx = m[2] * inv_np, uyy = m[3] * inv_np, uxy = m[4] * inv_np;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        acc += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
    const double total = block_sum<kT>(acc, sh);
    if (threadIdx.x == 0) ssim_parts[part] = total;
}

__global__ void __launch_bounds__(kT)
k_eval_finalize(uint32_t N, uint32_t B, uint32_t SB, float a_d, float a_r, float a_i, int mode, int mvl,
                const AnyPart *__restrict__ any_parts, const FramePart *__restrict__ frame_parts,
                const double *__restrict__ ssim_parts, double *__restrict__ acc, double *__restrict__ history,
                uint32_t max_frames) {
    __shared__ AnyPart sh_any;
    __shared__ float sh_mm[2][kT / 64];
    __shared__ double sh[kT / 64];
    const AnyPart tot = frame_any(any_parts, B, &sh_any);
    float gmin, gmax;
    frame_range(frame_parts, B, sh_mm, gmin, gmax);
    double s[10];
    for (int q = 0; q < 9; q++) {
        double v = 0.0;
        for (uint32_t i = threadIdx.x; i < B; i += kT) v += q < 6 ? frame_parts[i].s[q] : (double)frame_parts[i].a[q - 6];
        s[q] = block_sum<kT>(v, sh);
    }
    {
        double v = 0.0;
        for (uint32_t i = threadIdx.x; i < SB; i += kT) v += ssim_parts[i];
        s[9] = block_sum<kT>(v, sh);
    }
    if (threadIdx.x != 0) return;
    const uint32_t h = tot.nvalid ? tot.rmax - tot.rmin + 1 : 0u, w = tot.nvalid ? tot.cmax - tot.cmin + 1 : 0u;
    const double n = (double)N, nm = (double)tot.nvalid;
    double row[LNH_EVAL_SLOTS];
    row[LNH_EVAL_LOSS_DEPTH] = s[0] / n;
    row[LNH_EVAL_LOSS_RAYDROP] = s[1] / n;
    row[LNH_EVAL_LOSS_INTENSITY] = s[2] / n;
    row[LNH_EVAL_LOSS] = (double)a_d * row[LNH_EVAL_LOSS_DEPTH] + (double)a_r * row[LNH_EVAL_LOSS_RAYDROP] +
                         (double)a_i * row[LNH_EVAL_LOSS_INTENSITY];
    row[LNH_EVAL_MAE] = s[3] / nm;
    row[LNH_EVAL_RMSE] = sqrt(s[4] / nm);
    row[LNH_EVAL_DEPTH_RMSE] = sqrt(s[5] / nm);
    row[LNH_EVAL_A1] = s[6] / nm;
    row[LNH_EVAL_A2] = s[7] / nm;
    row[LNH_EVAL_A3] = s[8] / nm;
    row[LNH_EVAL_SSIM] = (h >= kWin && w >= kWin) ? s[9] / ((double)(h - kHalo) * (double)(w - kHalo)) : (double)NAN;
    row[LNH_EVAL_MASKED] = mask_applies(a_r, mode, tot.any != 0u) ? 1.0 : 0.0;
    row[LNH_EVAL_CROP_R0] = tot.nvalid ? (double)tot.rmin : 0.0;
    row[LNH_EVAL_CROP_C0] = tot.nvalid ? (double)tot.cmin : 0.0;
    row[LNH_EVAL_CROP_H] = (double)h;
    row[LNH_EVAL_CROP_W] = (double)w;
    row[LNH_EVAL_VALID] = nm;
    row[LNH_EVAL_DATA_RANGE] = (double)gmax - (double)gmin;
    row[LNH_EVAL_FRAMES] = 1.0;
    // a row the means cannot use: the valid pixels do not fill their rectangle (the reference's reshape raises, utils.py:
    // 949-956), or a number is not finite (no valid pixel, a rectangle below 7 x 7).  It is still added — the host refuses
    // an evaluation whose accumulator counts one (metrics.FrameEvaluator.measure)
    bool bad = mvl && nm != (double)h * (double)w;
    for (int q = LNH_EVAL_LOSS; q <= LNH_EVAL_SSIM; q++) bad = bad || !isfinite(row[q]);
    row[LNH_EVAL_BAD] = bad ? 1.0 : 0.0;
    const double frame = acc[LNH_EVAL_FRAMES];
    if (history && frame >= 0.0 && frame < (double)max_frames) {
        double *dst = history + (size_t)frame * LNH_EVAL_SLOTS;
        for (int q = 0; q < LNH_EVAL_SLOTS; q++) dst[q] = row[q];
    }
    for (int q = 0; q < LNH_EVAL_SLOTS; q++) acc[q] += row[q];
}

struct EvalWs {
    uint32_t B, tiles_r, tiles_c;
    uint64_t off_frame, off_ssim, bytes;
};

bool eval_ws(uint32_t H, uint32_t W, EvalWs &ws) {
    if (H < kWin || W < kWin || (uint64_t)H * W > (1u << 24)) return false;
    ws.B = div_up((uint64_t)H * W, kBlockPix);
    ws.tiles_r = div_up(H - kHalo, kTileR);
    ws.tiles_c = div_up(W - kHalo, kTileC);
    ws.off_frame = (uint64_t)ws.B * sizeof(AnyPart);
    ws.off_ssim = ws.off_frame + (uint64_t)ws.B * sizeof(FramePart);
    ws.bytes = ws.off_ssim + (uint64_t)ws.tiles_r * ws.tiles_c * sizeof(double);
    return true;
}

int eval_common(const char *who, uint32_t H, uint32_t W, int32_t mode, const void *workspace, uint64_t workspace_bytes,
                EvalWs &ws) {
    LNH_REQUIRE(H >= kWin && W >= kWin, LNH_ERR_INVALID_ARG, "%s: H (%u) and W (%u) must be at least 7 (the SSIM window)", who,
                H, W);
    LNH_REQUIRE((uint64_t)H * W <= (1u << 24), LNH_ERR_UNSUPPORTED, "%s: at most 2^24 pixels per frame (H %u, W %u)", who, H, W);
    LNH_REQUIRE(mode == LNH_EVAL_MODE_EVAL || mode == LNH_EVAL_MODE_TEST, LNH_ERR_INVALID_ARG,
                "%s: unknown mode %d (LNH_EVAL_MODE_EVAL 0, LNH_EVAL_MODE_TEST 1)", who, (int)mode);
    eval_ws(H, W, ws);
    LNH_REQUIRE(workspace && workspace_bytes >= ws.bytes && ((uintptr_t)workspace & 7) == 0, LNH_ERR_INVALID_ARG,
                "%s: workspace of %llu bytes, need %llu (8-byte aligned, not null)", who, (unsigned long long)workspace_bytes,
                (unsigned long long)ws.bytes);
    return LNH_OK;
}

int eval_options(const char *who, const lnh_lidar_loss_options *o) {
    LNH_REQUIRE(o, LNH_ERR_INVALID_ARG, "%s: null options pointer", who);
    const int32_t crit[3] = {o->depth_loss, o->raydrop_loss, o->intensity_loss};
    const char *slot[3] = {"depth", "raydrop", "intensity"};
    for (int i = 0; i < 3; i++) {
        LNH_REQUIRE(crit[i] != LNH_LOSS_COS, LNH_ERR_INVALID_ARG,
                    "%s: the cos criterion is a patch criterion, not a %s criterion (L1 0, MSE 1, HUBER 2, BCE 3)", who, slot[i]);
        LNH_REQUIRE(crit[i] >= LNH_LOSS_L1 && crit[i] <= LNH_LOSS_BCE, LNH_ERR_INVALID_ARG,
                    "%s: unknown %s criterion %d (L1 0, MSE 1, HUBER 2, BCE 3)", who, slot[i], (int)crit[i]);
    }
    LNH_REQUIRE(o->scale > 0.0f, LNH_ERR_INVALID_ARG, "%s: options scale must be positive (depths are compared in metres)", who);
    return LNH_OK;
}

}  // namespace

extern "C" {

uint64_t lnh_lidar_eval_workspace_bytes(uint32_t H, uint32_t W) {
    EvalWs ws;
    return eval_ws(H, W, ws) ? ws.bytes : 0;
}

int lnh_lidar_eval_frame(const float *image_lidar, const float *depth_lidar, const float *gt, uint32_t H, uint32_t W,
                         const lnh_lidar_loss_options *options, float intensity_inv_scale, int32_t mode, int32_t nerf_mvl,
                         void *workspace, uint64_t workspace_bytes, float *pred_intensity, float *pred_depth,
                         float *pred_mask, lnh_stream_t stream) {
    LNH_REQUIRE(image_lidar, LNH_ERR_INVALID_ARG, "lidar_eval_frame: null image_lidar pointer");
    LNH_REQUIRE(depth_lidar, LNH_ERR_INVALID_ARG, "lidar_eval_frame: null depth_lidar pointer");
    LNH_REQUIRE(pred_intensity && pred_depth && pred_mask, LNH_ERR_INVALID_ARG,
                "lidar_eval_frame: null output pointer (pred_intensity, pred_depth, pred_mask)");
    LNH_REQUIRE(gt || mode == LNH_EVAL_MODE_TEST, LNH_ERR_INVALID_ARG,
                "lidar_eval_frame: null gt pointer (only LNH_EVAL_MODE_TEST masks without a ground truth)");
    if (int rc = eval_options("lidar_eval_frame", options)) return rc;
    if (!gt) {
        LNH_REQUIRE(H >= 1 && W >= 1, LNH_ERR_INVALID_ARG, "lidar_eval_frame: H (%u) and W (%u) must be at least 1", H, W);
        LNH_REQUIRE((uint64_t)H * W <= (1u << 24), LNH_ERR_UNSUPPORTED,
                    "lidar_eval_frame: at most 2^24 pixels per call (H %u, W %u)", H, W);
        const uint32_t N = H * W;
        LNH_LAUNCH(k_eval_mask, dim3(div_up(N, kT)), dim3(kT), 0, (hipStream_t)stream, image_lidar, depth_lidar, N,
                   mask_applies(options->alpha_r, LNH_EVAL_MODE_TEST, false) ? 1 : 0, pred_intensity, pred_depth, pred_mask);
        return lnh_check_launch("lnh_lidar_eval_frame");
    }
    EvalWs ws;
    if (int rc = eval_common("lidar_eval_frame", H, W, mode, workspace, workspace_bytes, ws)) return rc;
    EvalArgs a{};
    a.image = image_lidar; a.depth = depth_lidar; a.gt = gt;
    a.H = H; a.W = W; a.N = H * W; a.B = ws.B;
    a.crit[0] = options->depth_loss; a.crit[1] = options->raydrop_loss; a.crit[2] = options->intensity_loss;
    a.delta = options->huber_delta; a.a_r = options->alpha_r; a.scale = options->scale; a.inv_i = intensity_inv_scale;
    a.mode = mode; a.mvl = nerf_mvl ? 1 : 0;
    AnyPart *any_parts = (AnyPart *)workspace;
    FramePart *frame_parts = (FramePart *)((char *)workspace + ws.off_frame);
    LNH_LAUNCH(k_eval_any, dim3(ws.B), dim3(kT), 0, (hipStream_t)stream, a, any_parts);
    LNH_LAUNCH(k_eval_frame, dim3(ws.B), dim3(kT), 0, (hipStream_t)stream, a, any_parts, frame_parts, pred_intensity,
               pred_depth, pred_mask);
    return lnh_check_launch("lnh_lidar_eval_frame");
}

int lnh_lidar_eval_ssim(const float *pred_depth, const float *gt, uint32_t H, uint32_t W, float scale, int32_t nerf_mvl,
                        void *workspace, uint64_t workspace_bytes, lnh_stream_t stream) {
    LNH_REQUIRE(pred_depth, LNH_ERR_INVALID_ARG, "lidar_eval_ssim: null pred_depth pointer");
    LNH_REQUIRE(gt, LNH_ERR_INVALID_ARG, "lidar_eval_ssim: null gt pointer");
    LNH_REQUIRE(scale > 0.0f, LNH_ERR_INVALID_ARG, "lidar_eval_ssim: scale must be positive");
    EvalWs ws;
    if (int rc = eval_common("lidar_eval_ssim", H, W, LNH_EVAL_MODE_EVAL, workspace, workspace_bytes, ws)) return rc;
    LNH_LAUNCH(k_eval_ssim, dim3(ws.tiles_c, ws.tiles_r), dim3(kT), 0, (hipStream_t)stream, pred_depth, gt, H, W, ws.B, scale,
               nerf_mvl ? 1 : 0, (const AnyPart *)workspace, (const FramePart *)((char *)workspace + ws.off_frame),
               (double *)((char *)workspace + ws.off_ssim));
    return lnh_check_launch("lnh_lidar_eval_ssim");
}

int lnh_lidar_eval_finalize(uint32_t H, uint32_t W, const lnh_lidar_loss_options *options, int32_t mode, int32_t nerf_mvl,
                            const void *workspace, uint64_t workspace_bytes, double *accumulator, double *history,
                            uint32_t max_frames, lnh_stream_t stream) {
    LNH_REQUIRE(accumulator, LNH_ERR_INVALID_ARG, "lidar_eval_finalize: null accumulator pointer");
    LNH_REQUIRE((((uintptr_t)accumulator | (uintptr_t)history) & 7) == 0, LNH_ERR_INVALID_ARG,
                "lidar_eval_finalize: accumulator and history must be 8-byte aligned");
    LNH_REQUIRE(history || max_frames == 0, LNH_ERR_INVALID_ARG, "lidar_eval_finalize: null history pointer with max_frames %u",
                max_frames);
    if (int rc = eval_options("lidar_eval_finalize", options)) return rc;
    EvalWs ws;
    if (int rc = eval_common("lidar_eval_finalize", H, W, mode, workspace, workspace_bytes, ws)) return rc;
    LNH_LAUNCH(k_eval_finalize, dim3(1), dim3(kT), 0, (hipStream_t)stream, H * W, ws.B, ws.tiles_r * ws.tiles_c,
               options->alpha_d, options->alpha_r, options->alpha_i, (int)mode, nerf_mvl ? 1 : 0,
               (const AnyPart *)workspace, (const FramePart *)((const char *)workspace + ws.off_frame),
               (const double *)((const char *)workspace + ws.off_ssim), accumulator, history, max_frames);
    return lnh_check_launch("lnh_lidar_eval_finalize");
}

}  // extern "C"
