// raydrop.hip — the ray-drop MLP of the PCGen baseline (lidarnvs/raydrop_train_pcgen.py: RayDrop, run_network with the identity
// embedding, img2mse / l1loss, torch.optim.Adam) in fp32: inference as one launch, a training step as three.
//   k_raydrop_rows   one workgroup per 16 rows: the whole network forward (first layer K = 5 and the one-column output as plain
//                    fmaf chains, the hidden layers on v_mfma_f32_16x16x4_f32, weights read where they are used), and for a
//                    training step the loss terms, the output gradient and the backward chain; every layer's activation and
//                    pre-activation gradient go to the workspace.  16 rows: a 2048-row batch covers 128 of the 256 CUs.
//   k_raydrop_wgrad  one workgroup per 16 x 16 tile of a weight gradient: dW = dY^T A over the WHOLE batch in row order (four
//                    waves take a quarter of the rows each, two interleaved MFMA chains per wave, added in a fixed order),
//                    divided by B once.  Its loop is branch-free with 16 operand loads in flight: it is bound by their latency.  Bias gradients ride along as a product with a column of ones.  The last workgroup
//                    adds the loss terms.  No partial sums in memory, no atomics: every gradient element has one owner.
//   k_raydrop_adam   torch.optim.Adam on the flat buffer, the step count and the learning-rate table on the device.
// Every sum's order is a function of (B, D, W) alone.
#include "common.h"

#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kRows = 16;  // rows per workgroup of k_raydrop_rows
constexpr int kIn = 5;     // direction x, y, z, depth, intensity

// offsets into the flat parameter buffer (floats)
__host__ __device__ inline uint64_t rd_hidden_w(uint32_t l, uint32_t W) {  // weight of hidden layer l >= 1
    return (uint64_t)(kIn + 1) * W + (uint64_t)(l - 1) * ((uint64_t)W * W + W);
}
__host__ __device__ inline uint64_t rd_out_w(uint32_t D, uint32_t W) { return rd_hidden_w(D, W); }
__host__ __device__ inline uint64_t rd_params(uint32_t D, uint32_t W) { return rd_out_w(D, W) + W + 1; }

struct RowsArgs {
    const float *params, *rows;
    uint32_t stride, N, D, loss_type;
    float *out;                          // inference
    float *acts, *dys, *dout, *partial;  // training: the workspace
    uint64_t plane;                      // floats per layer in acts / dys
};

template <int W, bool TRAIN>
__global__ void __launch_bounds__(256)
k_raydrop_rows(RowsArgs a) {
    constexpr int LD = W + 4, NT = W / 64;  // NT 16-column tiles per wave
    constexpr int kUnroll = W == 128 ? 8 : 4;  // k steps whose weight loads are in flight together (the loop is latency-bound)
    typedef float vec_t __attribute__((ext_vector_type(NT)));
    __shared__ __attribute__((aligned(16))) float buf[2][kRows * LD];
    __shared__ float xs[kRows][8];
    __shared__ float gs[kRows], es[kRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ci = lane & 15, kk = lane >> 4;
    const uint32_t row0 = blockIdx.x * kRows;
    if (tid < kRows * 8) {  // rows at or behind N are never read: they enter as zeros and leave nowhere
        const int r = tid >> 3, c = tid & 7;
        const uint32_t row = row0 + r;
        float v = 0.0f;
        if (row < a.N && c < (TRAIN ? kIn + 1 : kIn)) v = a.rows[(uint64_t)row * a.stride + c];
        xs[r][c] = v;
    }
    __syncthreads();
    float *cur = buf[0], *nxt = buf[1];
    {  // first layer, K = 5
        const float *w0 = a.params, *b0 = a.params + kIn * W;
        for (int idx = tid; idx < kRows * W; idx += 256) {
            const int r = idx / W, j = idx % W;
            float h = b0[j];
#pragma unroll
            for (int k = 0; k < kIn; k++) h = fmaf(xs[r][k], w0[j * kIn + k], h);
            h = fmaxf(h, 0.0f);
            cur[r * LD + j] = h;
            if (TRAIN && row0 + r < a.N) a.acts[(uint64_t)(row0 + r) * W + j] = h;
        }
    }
    __syncthreads();
    // hidden layers: H_l = relu(H_{l-1} W_l^T + b_l).  A operand: lane holds H[row ci][k], B operand: W_l[column ci of the tile][k],
    // with k = 16 t + 4 kk + c over the four MFMAs c of a step t (both operands are one 16-byte read)
    for (uint32_t l = 1; l < a.D; l++) {
        const float *wl = a.params + rd_hidden_w(l, W), *bl = wl + (uint64_t)W * W;
        f32x4 acc[NT];
        int jn[NT];
#pragma unroll
        for (int n = 0; n < NT; n++) {
            jn[n] = wave * (W / 4) + 16 * n + ci;
            const float b = bl[jn[n]];
            acc[n] = f32x4{b, b, b, b};
        }
#pragma unroll kUnroll
        for (int t = 0; t < W / 16; t++) {
            const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&cur[ci * LD + 16 * t + 4 * kk]);
            f32x4 b4[NT];
#pragma unroll
            for (int n = 0; n < NT; n++) b4[n] = *reinterpret_cast<const f32x4 *>(&wl[(uint64_t)jn[n] * W + 16 * t + 4 * kk]);
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int n = 0; n < NT; n++) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[c], b4[n][c], acc[n], 0, 0, 0);
        }
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int r = kk * 4 + reg;
                const float h = fmaxf(acc[n][reg], 0.0f);
                nxt[r * LD + jn[n]] = h;
                if (TRAIN && row0 + r < a.N) a.acts[l * a.plane + (uint64_t)(row0 + r) * W + jn[n]] = h;
            }
        __syncthreads();
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
    // output layer: 16 lanes per row, each a chain over every 16th unit, then a butterfly inside the 16 lanes
    const float *wo = a.params + rd_out_w(a.D, W);
    const int r = tid >> 4, s = tid & 15;
    const uint32_t row = row0 + r;
    float o = 0.0f;
#pragma unroll 4
    for (int m = 0; m < W / 16; m++) o = fmaf(cur[r * LD + s + 16 * m], wo[s + 16 * m], o);
    o += __shfl_xor(o, 8, 64);
    o += __shfl_xor(o, 4, 64);
    o += __shfl_xor(o, 2, 64);
    o += __shfl_xor(o, 1, 64);
    o += wo[W];
    if constexpr (!TRAIN) {
        if (s == 0 && row < a.N) a.out[row] = o;
    } else {
        const bool live = row < a.N;
        const float d = o - xs[r][kIn];
        float e, g;
        if (a.loss_type == 0) {
            e = d * d;
            g = 2.0f * d;
        } else {
            e = fabsf(d);
            g = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        }
        if (!live) e = g = 0.0f;
        if (s == 0) {
            es[r] = e;
            gs[r] = g;
            if (live) a.dout[row] = g;
        }
        __syncthreads();
        if (tid == 0) {
            float sum = 0.0f;
#pragma unroll
            for (int i = 0; i < kRows; i++) sum += es[i];
            a.partial[blockIdx.x] = sum;
        }
        // gradient at the last hidden layer's pre-activation, in place of its activation
        for (int idx = tid; idx < kRows * W; idx += 256) {
            const int r2 = idx / W, k = idx % W;
            const float v = cur[r2 * LD + k] > 0.0f ? gs[r2] * wo[k] : 0.0f;
            cur[r2 * LD + k] = v;
            if (row0 + r2 < a.N) a.dys[(a.D - 1) * a.plane + (uint64_t)(row0 + r2) * W + k] = v;
        }
        __syncthreads();
        // dY_{l-1} = (dY_l W_l) where H_{l-1} > 0.  A operand: dY_l[row ci][j], B operand: W_l[j][k] with j = 16 t + 4 kk + c;
        // the wave's columns are k = kb + n for tile n (NT consecutive floats per lane)
        for (uint32_t l = a.D - 1; l >= 1; l--) {
            const float *wl = a.params + rd_hidden_w(l, W);
            const int kb = wave * (W / 4) + NT * ci;
            f32x4 acc[NT];
#pragma unroll
            for (int n = 0; n < NT; n++) acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll kUnroll
            for (int t = 0; t < W / 16; t++) {
                const f32x4 a4 = *reinterpret_cast<const f32x4 *>(&cur[ci * LD + 16 * t + 4 * kk]);
                vec_t bv[4];
#pragma unroll
                for (int c = 0; c < 4; c++)
                    bv[c] = *reinterpret_cast<const vec_t *>(&wl[(uint64_t)(16 * t + 4 * kk + c) * W + kb]);
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int n = 0; n < NT; n++) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[c], bv[c][n], acc[n], 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int r2 = kk * 4 + reg;
                const bool in = row0 + r2 < a.N;
                const uint64_t at = (uint64_t)(row0 + r2) * W + kb;
                vec_t h, v;
#pragma unroll
                for (int n = 0; n < NT; n++) h[n] = 0.0f;
                if (in) h = *reinterpret_cast<const vec_t *>(&a.acts[(l - 1) * a.plane + at]);
#pragma unroll
                for (int n = 0; n < NT; n++) v[n] = h[n] > 0.0f ? acc[n][reg] : 0.0f;
                *reinterpret_cast<vec_t *>(&nxt[r2 * LD + kb]) = v;
                if (in) *reinterpret_cast<vec_t *>(&a.dys[(l - 1) * a.plane + at]) = v;
            }
            __syncthreads();
            float *t = cur;
            cur = nxt;
            nxt = t;
        }
    }
}

struct WgradArgs {
    const float *rows, *acts, *dys, *dout, *partial;
    uint32_t stride, B, D, n_partial;
    float *grad, *loss;
    uint64_t plane;
};

// Tiles: [0, T) the first layer (columns 0..4 the inputs, column 5 ones: its bias), then (D - 1) T^2 of the hidden matrices,
// then T of the output row (row 0 of the tile), then one workgroup for the loss.  T = W / 16.
template <int W>
__global__ void __launch_bounds__(256)
k_raydrop_wgrad(WgradArgs a) {
    constexpr uint32_t T = W / 16;
    __shared__ float red[4][256], redb[4][64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ci = lane & 15, kk = lane >> 4;
    const uint32_t n_hidden = (a.D - 1) * T * T;
    const uint32_t b = blockIdx.x;
    const float fB = (float)a.B;
    if (b == 2 * T + n_hidden) {  // the loss: lane i adds terms i, i + 64, ..., then the wave's butterfly; one division
        if (wave == 0) {
            float v = 0.0f;
            for (uint32_t i = lane; i < a.n_partial; i += 64) v += a.partial[i];
            v = wave_sum(v);
            if (lane == 0) *a.loss = v / fB;
        }
        return;
    }
    // role of this tile
    int kind;  // 0 first layer, 1 hidden, 2 output
    uint32_t l = 0, j0 = 0, k0 = 0;
    if (b < T) {
        kind = 0;
        j0 = 16 * b;
    } else if (b < T + n_hidden) {
        kind = 1;
        const uint32_t idx = b - T;
        l = 1 + idx / (T * T);
        j0 = 16 * ((idx % (T * T)) / T);
        k0 = 16 * (idx % T);
    } else {
        kind = 2;
        l = a.D;
        k0 = 16 * (b - T - n_hidden);
    }
    const bool with_bias = kind != 0 && k0 == 0;
    // Operands as (pointer, row stride, 0 / 1 mask, constant), so that the loop over the rows has no branch and a trip count that
    // depends on B alone: every load is unconditional from a clamped row (loads behind a branch wait for one another) and is
    // multiplied by the mask (x * 1 and x * 0 are exact).  A: dY[r][j0 + ci] (output layer: one column, lane 0 only).  B: the
    // layer's input [r][k0 + ci] (first layer: the five inputs, ones in column 5 for the bias, zeros behind).
    const float *ap = kind == 2 ? a.dout : a.dys + l * a.plane + j0 + ci;
    const uint32_t a_stride = kind == 2 ? 1 : W;
    const float a_mask = kind != 2 || ci == 0 ? 1.0f : 0.0f;
    const float *bp = kind == 0 ? a.rows + (ci < kIn ? ci : 0) : a.acts + (l - 1) * a.plane + k0 + ci;
    const uint32_t b_stride = kind == 0 ? a.stride : W;
    const float b_mask = kind != 0 || ci < kIn ? 1.0f : 0.0f;
    const float b_one = kind == 0 && ci == kIn ? 1.0f : 0.0f;
    const uint32_t chunk = ((a.B + 15) / 16) * 4;  // rows per wave, a multiple of 4
    const uint32_t trips = (chunk + 7) / 8;
    const uint32_t begin = wave * chunk, end = min(a.B, begin + chunk);
    f32x4 acc[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}}, accb[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
    auto rows_loop = [&](auto bias) {
        constexpr bool kBias = decltype(bias)::value;
        for (uint32_t i = 0; i < trips; i += 4) {  // 32 rows a trip: 16 loads in flight, then two chains of alternating 4-row steps
            float av[8], bv[8], in[8];
#pragma unroll
            for (int h = 0; h < 8; h++) {
                const uint32_t r = begin + 8 * i + 4 * h + kk;
                in[h] = r < end ? 1.0f : 0.0f;  // (a row at or behind the end adds 0 * 0; row B - 1 is read in its place)
                const uint32_t rr = r < end ? r : a.B - 1;
                av[h] = ap[(uint64_t)rr * a_stride];
                bv[h] = bp[(uint64_t)rr * b_stride];
            }
#pragma unroll
            for (int h = 0; h < 8; h++) {
                const float x = av[h] * (in[h] * a_mask), y = bv[h] * (in[h] * b_mask) + in[h] * b_one;
                acc[h & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc[h & 1], 0, 0, 0);
                if constexpr (kBias) accb[h & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, in[h], accb[h & 1], 0, 0, 0);
            }
        }
    };
    if (with_bias) rows_loop(std::true_type{});
    else rows_loop(std::false_type{});
    // C layout: column (k) = ci, row (j) = 4 kk + reg
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        red[wave][(kk * 4 + reg) * 16 + ci] = acc[0][reg] + acc[1][reg];
        if (with_bias && ci == 0) redb[wave][kk * 4 + reg] = accb[0][reg] + accb[1][reg];
    }
    __syncthreads();
    const uint32_t jr = tid >> 4, kc = tid & 15;
    const float v = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / fB;
    if (kind == 0) {
        if (kc < kIn) a.grad[(uint64_t)(j0 + jr) * kIn + kc] = v;
        else if (kc == kIn) a.grad[(uint64_t)kIn * W + j0 + jr] = v;
    } else if (kind == 1) {
        a.grad[rd_hidden_w(l, W) + (uint64_t)(j0 + jr) * W + k0 + kc] = v;
    } else if (jr == 0) {
        a.grad[rd_out_w(a.D, W) + k0 + kc] = v;
    }
    if (with_bias && tid < (kind == 2 ? 1u : 16u)) {
        const float vb = ((redb[0][tid] + redb[1][tid]) + (redb[2][tid] + redb[3][tid])) / fB;
        if (kind == 1) a.grad[rd_hidden_w(l, W) + (uint64_t)W * W + j0 + tid] = vb;
        else a.grad[rd_out_w(a.D, W) + W] = vb;
    }
}

struct RdAdamArgs {
    float *p, *m, *v;
    const float *g;
    uint32_t n, lr_len;
    const float *lr_table, *step_in;
    float *step_out;
    double beta1, beta2, eps;
};

// the arithmetic of k_adam_table (optim.hip): moments with double weights, the parameter update in fp32
__global__ void __launch_bounds__(256)
k_raydrop_adam(RdAdamArgs a) {
    const float t0 = *a.step_in, t = t0 + 1.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.step_out = t;  // double-buffered step counter
    const uint32_t at = t0 < (float)(a.lr_len - 1) ? (uint32_t)t0 : a.lr_len - 1;
    const double lr = (double)a.lr_table[at];
    const double bc1 = 1.0 - pow(a.beta1, (double)t), bc2 = 1.0 - pow(a.beta2, (double)t);
    const double w1 = 1.0 - a.beta1, w2 = 1.0 - a.beta2;
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2), eps = (float)a.eps;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
        const float g = a.g[i];
        float m = a.m[i], v = a.v[i];
        m = (float)((double)m + w1 * ((double)g - (double)m));
        v = (float)(a.beta2 * (double)v + w2 * (double)g * (double)g);
        a.m[i] = m;
        a.v[i] = v;
        a.p[i] -= step_size * m / (sqrtf(v) / bc2_sqrt + eps);
    }
}

bool shape_ok(uint32_t D, uint32_t W) { return (W == 128 || W == 256) && D >= 1 && D <= 8; }

}  // namespace

extern "C" {

uint64_t lnh_raydrop_param_count(uint32_t D, uint32_t W) { return shape_ok(D, W) ? rd_params(D, W) : 0; }

uint64_t lnh_raydrop_workspace_size(uint32_t D, uint32_t W, uint32_t B) {
    if (!shape_ok(D, W) || B == 0 || B > (1u << 24)) return 0;
    const uint64_t bpad = ((uint64_t)B + kRows - 1) / kRows * kRows;
    return (2 * (uint64_t)D * W * bpad + bpad + bpad / kRows) * sizeof(float);
}

int lnh_raydrop_forward(const float *params, uint32_t D, uint32_t W, const float *rows, uint32_t stride, uint32_t N, float *out,
                        lnh_stream_t stream) {
    LNH_REQUIRE(shape_ok(D, W), LNH_ERR_INVALID_ARG, "raydrop_forward: W must be 128 or 256 and 1 <= D <= 8 (got D %u, W %u)", D, W);
    LNH_REQUIRE(stride >= kIn, LNH_ERR_INVALID_ARG, "raydrop_forward: rows need at least 5 columns (stride %u)", stride);
    LNH_REQUIRE(params && (N == 0 || (rows && out)), LNH_ERR_INVALID_ARG, "raydrop_forward: null pointer");
    LNH_REQUIRE(((uintptr_t)params & 15) == 0, LNH_ERR_INVALID_ARG, "raydrop_forward: params must be 16-byte aligned");
    LNH_REQUIRE(N <= 0xfffffff0u - kRows, LNH_ERR_INVALID_ARG, "raydrop_forward: too many rows");
    if (N == 0) return LNH_OK;
    RowsArgs a{};
    a.params = params; a.rows = rows; a.stride = stride; a.N = N; a.D = D; a.out = out;
    const dim3 grid((N + kRows - 1) / kRows);
    if (W == 128) LNH_LAUNCH((k_raydrop_rows<128, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else LNH_LAUNCH((k_raydrop_rows<256, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_raydrop_forward");
}

int lnh_raydrop_grad(const float *params, uint32_t D, uint32_t W, const float *rows, uint32_t B, uint32_t loss_type, void *ws,
                     uint64_t ws_bytes, float *loss, float *grad, lnh_stream_t stream) {
    LNH_REQUIRE(shape_ok(D, W), LNH_ERR_INVALID_ARG, "raydrop_grad: W must be 128 or 256 and 1 <= D <= 8 (got D %u, W %u)", D, W);
    LNH_REQUIRE(params && rows && loss && grad && ws, LNH_ERR_INVALID_ARG, "raydrop_grad: null pointer");
    LNH_REQUIRE(B >= 1 && B <= (1u << 24), LNH_ERR_INVALID_ARG, "raydrop_grad: batch of %u rows (1 .. 2^24)", B);
    LNH_REQUIRE(loss_type <= 1, LNH_ERR_INVALID_ARG, "raydrop_grad: loss_type %u (0 mse, 1 l1)", loss_type);
    LNH_REQUIRE((((uintptr_t)params | (uintptr_t)ws) & 15) == 0, LNH_ERR_INVALID_ARG,
                "raydrop_grad: params and workspace must be 16-byte aligned");
    const uint64_t need = lnh_raydrop_workspace_size(D, W, B);
    LNH_REQUIRE(ws_bytes >= need, LNH_ERR_INVALID_ARG, "raydrop_grad: workspace of %llu bytes, %llu needed",
                (unsigned long long)ws_bytes, (unsigned long long)need);
    const uint64_t bpad = ((uint64_t)B + kRows - 1) / kRows * kRows;
    RowsArgs a{};
    a.params = params; a.rows = rows; a.stride = kIn + 1; a.N = B; a.D = D; a.loss_type = loss_type;
    a.plane = bpad * W;
    a.acts = (float *)ws;
    a.dys = a.acts + D * a.plane;
    a.dout = a.dys + D * a.plane;
    a.partial = a.dout + bpad;
    const uint32_t tiles = (uint32_t)(bpad / kRows);
    WgradArgs g{};
    g.rows = rows; g.acts = a.acts; g.dys = a.dys; g.dout = a.dout; g.partial = a.partial;
    g.stride = kIn + 1; g.B = B; g.D = D; g.n_partial = tiles; g.grad = grad; g.loss = loss; g.plane = a.plane;
    const uint32_t T = W / 16;
    const dim3 wgrid(2 * T + (D - 1) * T * T + 1);
    if (W == 128) {
        LNH_LAUNCH((k_raydrop_rows<128, true>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
        LNH_LAUNCH((k_raydrop_wgrad<128>), wgrid, dim3(256), 0, (hipStream_t)stream, g);
    } else {
        LNH_LAUNCH((k_raydrop_rows<256, true>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
        LNH_LAUNCH((k_raydrop_wgrad<256>), wgrid, dim3(256), 0, (hipStream_t)stream, g);
    }
    return lnh_check_launch("lnh_raydrop_grad");
}

int lnh_raydrop_adam(float *params, float *exp_avg, float *exp_avg_sq, const float *grad, uint32_t P, const float *lr_table,
                     uint32_t lr_len, const float *step_in, float *step_out, double beta1, double beta2, double eps,
                     lnh_stream_t stream) {
    LNH_REQUIRE(params && exp_avg && exp_avg_sq && grad && lr_table && step_in && step_out, LNH_ERR_INVALID_ARG,
                "raydrop_adam: null pointer");
    LNH_REQUIRE(step_in != step_out, LNH_ERR_INVALID_ARG, "raydrop_adam: the step counter is double-buffered");
    LNH_REQUIRE(lr_len >= 1 && lr_len <= (1u << 24), LNH_ERR_INVALID_ARG, "raydrop_adam: learning-rate table of %u entries", lr_len);
    if (P == 0) return LNH_OK;
    RdAdamArgs a{params, exp_avg, exp_avg_sq, grad, P, lr_len, lr_table, step_in, step_out, beta1, beta2, eps};
    const uint32_t blocks = (P + 255) / 256 < 1024 ? (P + 255) / 256 : 1024;
    LNH_LAUNCH(k_raydrop_adam, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return lnh_check_launch("lnh_raydrop_adam");
}

}  // extern "C"
