/*
 * lidarnerf_hip.h — C ABI of liblidarnerf_hip.so, the MI355X (gfx950) implementation of the LiDAR-NeRF
 * train/render hot path: hash-grid / SH / frequency encodings, fused tiny MLP, per-ray compositing, occupancy
 * indexing — forward and backward.
 *
 * Conventions (every entry point):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer owned by the caller unless its name ends in
 *     `_host` (the caller allocates every output, exactly as the reference's pybind layer does, e.g.
 *     lidarnerf/gridencoder/grid.py:60-67, lidarnerf/raymarching/raymarching.py:235-245);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); kernels are enqueued, never synchronised;
 *   - returns LNH_OK (0) or a negative LNH_ERR_*; never throws, never allocates device memory;
 *     lnh_last_error() returns a thread-local message for the last failure (the reference raises TORCH_CHECK /
 *     std::runtime_error for the same conditions, e.g. gridencoder.cu:430,476,608-624);
 *   - re-entrant: no global state (the reference's ffmlp keeps static stream/event vectors, ffmlp.cu:1020-1049).
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference repo root).
 */
#ifndef LIDARNERF_HIP_H
#define LIDARNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNH_API __attribute__((visibility("default")))

typedef void *lnh_stream_t;

enum { LNH_OK = 0, LNH_ERR_INVALID_ARG = -1, LNH_ERR_UNSUPPORTED = -2, LNH_ERR_LAUNCH = -3 };

/* element type of tables / activations */
enum { LNH_F32 = 0, LNH_F16 = 1 };

/* activations, numbering of lidarnerf/ffmlp/ffmlp.py:170-184 (convert_activation) */
enum {
    LNH_ACT_RELU = 0, LNH_ACT_EXPONENTIAL = 1, LNH_ACT_SINE = 2, LNH_ACT_SIGMOID = 3,
    LNH_ACT_SQUAREPLUS = 4, LNH_ACT_SOFTPLUS = 5, LNH_ACT_NONE = 6
};

#define LNH_MAX_LEVELS 32

/* 100: the initial ABI.  101 adds gridtype 2 (tiny-cuda-nn's HashGrid lattice, below) to every grid entry point that takes
 * a gridtype, and lnh_grid_encode_forward_mapped_ex.  102 adds lnh_lidar_loss_ex (every loss option of the reference CLI). */
LNH_API int lnh_version(void);
LNH_API const char *lnh_last_error(void);
/* "gfx950" — the only architecture this library carries code for */
LNH_API const char *lnh_arch(void);
/* "product" for the shipped library; timing-probe builds (tools/probe_variants.py) report their own name here and the
 * Python side refuses to load them unless LNH_ALLOW_VARIANT=1 — results of such builds are wrong by construction. */
LNH_API const char *lnh_build_variant(void);

/* ------------------------------------------------------------------ hash / tiled grid encoder --------------- */
/*
 * Replaces grid_encode_forward   lidarnerf/gridencoder/src/gridencoder.h:12-25 (gridencoder.cu:594-637).
 * inputs [B,D] f32 in [0,1]; embeddings [rows,C] (dtype); offsets_host [L+1] int32 ON THE HOST (the reference
 * passes a device tensor that never changes after construction: grid.py:179-193; a binding caches offsets.cpu());
 * outputs [L,B,C] (dtype) — level-major exactly like the reference (gridencoder.cu:437-438);
 * dy_dx NULL or [B,L,D,C] (dtype).  D in {2,3,4,5}, C in {1,2,4,8}; gridtype 0=hash 1=tiled 2=hash on tiny-cuda-nn's
 * lattice; interp 0=linear 1=smoothstep.  S = log2(per_level_scale), H = base resolution.
 *
 * gridtype 2 (since lnh_version 101) restates tiny-cuda-nn's published GridEncoding (parity with a real tiny-cuda-nn build
 * is UNPINNED): scale, resolution, cell position and hash as gridtype 0, but a dense level has stride `resolution` (not
 * resolution + 1), res^D rows rounded up to 8, and its row index is ALWAYS taken modulo the level's rows — the vertices at
 * x = resolution alias the next row.  align_corners != 0 with gridtype 2 returns LNH_ERR_INVALID_ARG; so does a gridtype
 * above 2, in every entry point that takes one.  Points outside [0,1] give zero output and no gradient (tiny-cuda-nn does
 * not check).
 */
LNH_API int lnh_grid_encode_forward(const float *inputs, const void *embeddings, const int32_t *offsets_host,
                                    void *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                    uint32_t H, void *dy_dx, uint32_t gridtype, int align_corners, uint32_t interp,
                                    int dtype, lnh_stream_t stream);
/* Scheduling knob of the three forward entry points, process-wide; never changes a result.  The forward's workgroups run
 * level-major (all of level 0, then level 1, ...) except for up to `max_pairs` PAIRS of levels — the finest hashed level
 * with the coarsest level, the next finest with the next coarsest, ... — whose workgroups alternate in blocks of `block`
 * consecutive ids (rounded up to a power of two in 8 .. 1024; 0 = the default block, 32).  A pair needs a fine level of the
 * plain hashed class (power-of-two table, linear interpolation, align_corners off) and a partner that is hashed or dense
 * in every dimension.  max_pairs = 0: plain level-major order.  max_pairs = 0xffffffff, the default: the default block, and
 * as many pairs as have a fine level of at least 32 times its partner's resolution (5 pairs for 16 levels from 16 to
 * 32768).  The environment variable LNH_FWD_SCHEDULE = "max_pairs[,block]", read at the first forward call, sets the same
 * two numbers unless this function was called before. */
LNH_API void lnh_grid_forward_set_schedule(uint32_t max_pairs, uint32_t block);
/*
 * Replaces grid_encode_backward  gridencoder.h:26-41 (gridencoder.cu:639-693).
 * grad [L,B,C] (dtype); grad_embeddings [rows,C] (dtype), ZERO-INITIALISED by the caller (grid.py:106), receives
 * atomic scatter-adds; dy_dx / grad_inputs NULL or [B,L,D,C] / [B,D] (dtype).  `embeddings` is unused by the
 * arithmetic (kept for signature parity, may be NULL).
 */
LNH_API int lnh_grid_encode_backward(const void *grad, const float *inputs, const void *embeddings,
                                     const int32_t *offsets_host, void *grad_embeddings, uint32_t B, uint32_t D,
                                     uint32_t C, uint32_t L, float S, uint32_t H, const void *dy_dx, void *grad_inputs,
                                     uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                     lnh_stream_t stream);
/*
 * Same result as lnh_grid_encode_backward for the hot configuration (D == 3, C == 2) without a single atomic add to
 * HBM: contributions are binned per 8192-row table bucket in a caller-provided workspace and reduced in LDS in 64-bit
 * fixed point (grid_pool.h, "bucketed backward"): the result is one integer sum per table row, independent of execution
 * order (bit-reproducible run to run), rounded once to the table type.  `workspace` is scratch device memory of at least
 * lnh_grid_backward_workspace_size(...) bytes (0 = configuration not supported by this path); its content is
 * irrelevant before and after the call.  No dy_dx / grad_inputs (LiDAR sample positions carry no gradient).
 */
LNH_API uint64_t lnh_grid_backward_workspace_size(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C,
                                                  uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                                  int align_corners, int dtype);
/* The workspace serves one chunk of the batch at a time: any size between lnh_grid_backward_workspace_size_min(...) and
 * lnh_grid_backward_workspace_size(...) is accepted — a smaller workspace means shorter chunks (more launches: 3.09 / 1.60 /
 * 0.91 GB cost 897 / 922 / 992 us at 4096 rays x 832 samples), never another result class.  Below the minimum the call
 * returns LNH_ERR_INVALID_ARG and lnh_last_error() names the minimum. */
LNH_API uint64_t lnh_grid_backward_workspace_size_min(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C,
                                                      uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                                      int align_corners, int dtype);
/* Testing knob, process-wide: entries per reduce slice (0 restores the default, 512 K; clamped to [1024, 512 K]) — with the
 * default only a concentrated batch of more than half a million entries per bucket is reduced in slices; a small value
 * lets the tests reach that path with small inputs.  Set it BEFORE lnh_grid_backward_workspace_size (more slices need
 * more image slots).  Never changes a result. */
LNH_API void lnh_grid_backward_set_slice_entries(uint32_t entries);
/* Host-side description of that workspace's bucket plan for `level` (no device work): out[0] = table buckets of the
 * level, out[1] = pool slots per bucket (what exceeds them goes to the level's spill list), out[2] = rows per bucket,
 * out[3] = entries per reduce slice (a bucket with more is reduced by several workgroups).  The sum the call produces
 * never depends on these numbers — integer accumulation (see grid_pool.h) — the tests use them to build inputs that
 * overflow a bucket by a few entries or split one.  Returns LNH_ERR_UNSUPPORTED where workspace_size returns 0. */
LNH_API int lnh_grid_backward_plan_info(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                        float S, uint32_t H, uint32_t gridtype, int align_corners, int dtype,
                                        uint32_t level, uint32_t *out4);
/* The bucketed backward.  One implementation, lnh_grid_encode_backward_ws_ex; the four entry points after it forward to it.
 *   level_begin, level_end   only the levels [level_begin, level_end) are worked on; rows of other levels are not touched.
 *          level_end > L is clamped to L; level_begin > level_end returns LNH_ERR_INVALID_ARG.
 *   split  0: the whole backward of those levels.
 *          1 ("begin"): everything except the reduce pass of the (last) chunk, for ALL levels (the window is checked, then
 *          ignored); 2 ("finish"): that reduce pass for the levels of the window, after which their rows of grad_embeddings
 *          are final.  A data-parallel caller runs begin once, then finish for consecutive windows covering [0, L), with the
 *          same arguments and the same workspace on the same stream: the gradient of a finished window can go to the
 *          all-reduce while the next window is being reduced, and the scatter pass is NOT cut into windows (which costs it a
 *          quarter of its speed).  The result is bit-identical to split 0.
 *   flags  for a caller that has just cleared its buffers itself (a training step that clears every accumulated-into buffer
 *          of its backward pass with one lnh_zero_regions launch); a caller that sets one without having cleared gets garbage.
 *          LNH_BWD_WS_CLEARED: the first lnh_grid_backward_workspace_clear_bytes(...) bytes of `workspace` are zero on
 *          entry (the cursors of the batch's FIRST chunk: that chunk's clear launch is skipped);
 *          LNH_BWD_TABLE_ZERO: grad_embeddings holds zeros on entry — the reduce pass of the first chunk stores its sums
 *          instead of adding them to rows it would have to read first (the same values: 0 + x).
 * lnh_grid_backward_workspace_clear_bytes: size of that head for the chunk plan the call will choose for `workspace_bytes`
 * (0: unsupported configuration / workspace too small). */
#define LNH_BWD_WS_CLEARED 1u
#define LNH_BWD_TABLE_ZERO 2u
LNH_API int lnh_grid_encode_backward_ws_ex(const void *grad, const float *inputs, const int32_t *offsets_host,
                                           void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                           uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                           void *workspace, uint64_t workspace_bytes, uint32_t level_begin,
                                           uint32_t level_end, int split, uint32_t flags, lnh_stream_t stream);
LNH_API uint64_t lnh_grid_backward_workspace_clear_bytes(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C,
                                                         uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                                         int align_corners, uint32_t interp, int dtype,
                                                         uint64_t workspace_bytes);
/* = lnh_grid_encode_backward_ws_ex(..., 0, L, 0, 0): all levels in one call. */
LNH_API int lnh_grid_encode_backward_ws(const void *grad, const float *inputs, const int32_t *offsets_host,
                                        void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                        uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                        void *workspace, uint64_t workspace_bytes, lnh_stream_t stream);
/* = ..._ws_ex(..., level_begin, level_end, 0, 0), except that level_end > L returns LNH_ERR_INVALID_ARG (not clamped). */
LNH_API int lnh_grid_encode_backward_ws_levels(const void *grad, const float *inputs, const int32_t *offsets_host,
                                               void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                               float S, uint32_t H, uint32_t gridtype, int align_corners,
                                               uint32_t interp, int dtype, void *workspace, uint64_t workspace_bytes,
                                               uint32_t level_begin, uint32_t level_end, lnh_stream_t stream);
/* = ..._ws_ex(..., 0, L, 1, 0). */
LNH_API int lnh_grid_encode_backward_ws_begin(const void *grad, const float *inputs, const int32_t *offsets_host,
                                              void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                              float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp,
                                              int dtype, void *workspace, uint64_t workspace_bytes, lnh_stream_t stream);
/* = ..._ws_ex(..., level_begin, level_end, 2, 0), except that level_end > L returns LNH_ERR_INVALID_ARG (not clamped). */
LNH_API int lnh_grid_encode_backward_ws_finish(const void *grad, const float *inputs, const int32_t *offsets_host,
                                               void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                               float S, uint32_t H, uint32_t gridtype, int align_corners,
                                               uint32_t interp, int dtype, void *workspace, uint64_t workspace_bytes,
                                               uint32_t level_begin, uint32_t level_end, lnh_stream_t stream);
/*
 * Replaces grad_total_variation  gridencoder.h:43-55 (gridencoder.cu:695-910): adds the TV-regulariser gradient
 * of the cells visited by `inputs` into `grad` (same layout as embeddings).
 */
LNH_API int lnh_grad_total_variation(const void *inputs, const void *embeddings, void *grad,
                                     const int32_t *offsets_host, float weight, uint32_t B, uint32_t D, uint32_t C,
                                     uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, int dtype,
                                     lnh_stream_t stream);
/*
 * Bit-exact contract of get_grid_index / fast_hash (gridencoder.cu:53-93): element index (row*C) of the 2^D
 * corners of every (level, point); out_idx [L,B,2^D] uint32, 0xffffffff for out-of-range points.
 */
LNH_API int lnh_grid_corner_indices(const float *inputs, const int32_t *offsets_host, uint32_t *out_idx, uint32_t B,
                                    uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                    int align_corners, lnh_stream_t stream);

/* ------------------------------------------------------------------ frequency encoder ----------------------- */
/* Replaces freq_encode_forward   lidarnerf/freqencoder/src/freqencoder.h:8-14 (freqencoder.cu:103-122).
 * inputs [B,D] f32 -> outputs [B,C] f32, C = D + 2*D*deg, layout [x | sin(2^f x) | cos(2^f x)]_f. */
LNH_API int lnh_freq_encode_forward(const float *inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                                    float *outputs, lnh_stream_t stream);
/* Replaces freq_encode_backward  freqencoder.h:16-22 (freqencoder.cu:124-147); uses the SAVED outputs. */
LNH_API int lnh_freq_encode_backward(const float *grad, const float *outputs, uint32_t B, uint32_t D, uint32_t deg,
                                     uint32_t C, float *grad_inputs, lnh_stream_t stream);

/* ------------------------------------------------------------------ spherical-harmonics encoder -------------- */
/* Replaces sh_encode_forward     lidarnerf/shencoder/src/shencoder.h:9-14 (shencoder.cu:887-912).
 * inputs [B,3] f32 (raw direction) -> outputs [B,degree^2] f32; dy_dx NULL or [B,3,degree^2]. degree in 1..4. */
LNH_API int lnh_sh_encode_forward(const float *inputs, float *outputs, uint32_t B, uint32_t D, uint32_t degree,
                                  float *dy_dx, lnh_stream_t stream);
/* Replaces sh_encode_backward    shencoder.h:15-20 (shencoder.cu:914-943): grad_inputs[b,d] += sum grad*dy_dx. */
LNH_API int lnh_sh_encode_backward(const float *grad, const float *inputs, uint32_t B, uint32_t D, uint32_t degree,
                                   const float *dy_dx, float *grad_inputs, lnh_stream_t stream);

/* ------------------------------------------------------------------ fully fused MLP -------------------------- */
/*
 * Replaces ffmlp_forward / ffmlp_inference / ffmlp_backward  lidarnerf/ffmlp/src/ffmlp.h:7-44
 * (ffmlp.cu:866-1263) and the bias-free Linear stacks of lidarnerf/nerf/network.py:45-99.
 * inputs [B,input_dim] f16; weights flat f16: [hidden*input | hidden*hidden*n_hidden_mats | output_dim*hidden],
 * every matrix row-major [out,in] (ffmlp.py:222-226 with n_hidden_mats = num_layers-1; n_hidden_mats = 0 gives
 * the 2-matrix sigma net).  output_dim is the PADDED width (multiple of 16, <= 16 for the fused path);
 * outputs [B,output_dim] f16.  forward_buffer NULL (inference) or [n_hidden_mats+1, B, hidden] f16 receiving the
 * post-activation of every hidden layer (ffmlp.py:43-58).  Accumulation is fp32 on MFMA (the reference
 * accumulates in fp16 WMMA fragments, ffmlp.cu:788-791).  B must be a multiple of 16.
 */
LNH_API int lnh_mlp_forward(const void *inputs, const void *weights, uint32_t B, uint32_t input_dim,
                            uint32_t output_dim, uint32_t hidden_dim, uint32_t n_hidden_mats, uint32_t activation,
                            uint32_t output_activation, void *forward_buffer, void *outputs, lnh_stream_t stream);
/*
 * Weight gradients of the MLP family are FIXED-ORDER sums: every backward kernel leaves one partial sum per workgroup in
 * `wgrad_ws` and a second, small launch on the same stream adds the partials up in workgroup-index order and adds the result
 * to the gradient (csrc/wgrad.h) — the same bits on every run, as with the reference's split-K GEMMs (ffmlp.cu:1107-1142);
 * rounds 1-5 used fp32 device atomics, whose order changed from run to run.
 * wgrad_ws: device scratch of lnh_wgrad_workspace_bytes() bytes, 16-byte aligned, contents irrelevant; one workspace serves
 * all launches of a stream, launches that may overlap in time (several streams) need one each.  Taken by lnh_mlp_backward,
 * lnh_density_mlp_backward, lnh_lidar_color_backward(_image), lnh_ragged_color_backward, lnh_lidar_dir_term_backward and
 * their _bf16 builds.
 */
LNH_API uint64_t lnh_wgrad_workspace_bytes(void);
/*
 * grad [B,output_dim] f16; grad_weights: f32 flat vector (same ordering as weights, 16-byte aligned): the batch's sum is
 * ADDED to it (clear it first for a plain gradient); grad_inputs NULL or [B,input_dim] f16.
 * The hidden activations are recomputed from `inputs` (no forward_buffer needed).
 */
LNH_API int lnh_mlp_backward(const void *grad, const void *inputs, const void *weights, uint32_t B,
                             uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t n_hidden_mats,
                             uint32_t activation, uint32_t output_activation, void *grad_inputs, float *grad_weights,
                             void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);

/*
 * Shapes.  hidden_dim 32 / 64 with n_hidden_mats <= 2: register-resident kernels, and lnh_mlp_backward is ONE kernel.
 * hidden_dim 128 / 256 (ffmlp.cu:756-800) and n_hidden_mats 3 .. 14 at any of the four widths: lnh_mlp_forward runs
 * kernels that load a weight fragment where it is used (csrc/mlp_wide.hip); the backward is the reference's own split
 * (ffmlp.cu:578-733 fused activation gradients + 1107-1263 split-K GEMMs for the weights):
 *   lnh_mlp_backward_data: from grad [B,output_dim], the forward_buffer lnh_mlp_forward filled, and weights_t — the
 *     matrices TRANSPOSED, flat [input*hidden (W0^T, rows = inputs) | hidden*hidden*n_hidden_mats (each Wh^T) |
 *     hidden*output_dim (Wo^T, rows = hidden units)] — writes backward_buffer [n_hidden_mats+1, B, hidden] f16 =
 *     dL/d(pre-activation) of every hidden layer and grad_inputs (NULL or [B,input_dim]);
 *   the weight gradients are the GEMMs dW0 = backward_buffer[0]^T inputs, dWh_m = backward_buffer[m+1]^T
 *     forward_buffer[m], dWo = grad^T forward_buffer[n_hidden_mats]: one lnh_mlp_wgrad call each (below).
 *   lnh_mlp_backward returns LNH_ERR_UNSUPPORTED for these shapes and says so.  Works for the narrow shapes too.
 * hidden_dim 16 has no kernel of its own (the module zero-pads it onto 32); input_dim > 128: LNH_ERR_UNSUPPORTED.
 */
LNH_API int lnh_mlp_backward_data(const void *grad, const void *forward_buffer, const void *weights_t, uint32_t B,
                                  uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t n_hidden_mats,
                                  uint32_t activation, void *backward_buffer, void *grad_inputs, lnh_stream_t stream);
/*
 * Weight gradient of ONE layer of a wide fused MLP, the contraction over the batch the reference runs as a split-K CUTLASS
 * GEMM (ffmlp.cu:1107-1263, cutlass_matmul.h:481-616):  grad_weights[M, N] += grad^T acts,  grad [B, M] and acts [B, N] f16
 * (row-major; rows of lnh_mlp_backward_data's backward_buffer / lnh_mlp_forward's forward_buffer / the MLP input), M and N
 * multiples of 16 in 16 .. 256, grad_weights f32 row-major (a slice of the flat gradient vector), 16-byte aligned pointers.
 * Fixed-order sum over the batch (wgrad_ws: lnh_wgrad_workspace_bytes): the same bits on every run.
 */
LNH_API int lnh_mlp_wgrad(const void *grad, const void *acts, uint32_t B, uint32_t M, uint32_t N, float *grad_weights,
                          void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);

/* ------------------------------------------------------------------ ray utilities / occupancy grid ----------- */
/* Replaces near_far_from_aabb    lidarnerf/raymarching/src/raymarching.h:6-12 (raymarching.cu:104-177). */
LNH_API int lnh_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N,
                                   float min_near, float *nears, float *fars, lnh_stream_t stream);
/* What NeRFRenderer.run_cuda does in front of the marcher, in ONE launch (no pybind counterpart: the reference's
 * renderer does it with torch ops — renderer.py:129-138 for the LiDAR range; this build's run_cuda cuts it at the box):
 *   nears[n] = near;  fars[n] = torch.minimum(near * far_factor, far of lnh_near_far_from_aabb(rays_o, rays_d, aabb, near))
 * (bit for bit, NaN exits included), and up to 4 device regions cleared (the marcher's zero-initialised sample buffers —
 * raymarching.py:235-245 —, its counter, the colour buffer): host arrays of pointers and byte counts, 4-byte granular. */
LNH_API int lnh_lidar_march_prologue(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N, float near,
                                     float far_factor, float *nears, float *fars, void *const *zero_ptrs,
                                     const uint64_t *zero_bytes, uint32_t zero_count, lnh_stream_t stream);
/* Replaces sph_from_ray          raymarching.h:13-17 (raymarching.cu:182-231). */
LNH_API int lnh_sph_from_ray(const float *rays_o, const float *rays_d, float radius, uint32_t N, float *coords,
                             lnh_stream_t stream);
/* Replaces morton3D / morton3D_invert  raymarching.h:18-21 (raymarching.cu:71-95,237-279) — bit exact. */
LNH_API int lnh_morton3D(const int32_t *coords, uint32_t N, int32_t *indices, lnh_stream_t stream);
LNH_API int lnh_morton3D_invert(const int32_t *indices, uint32_t N, int32_t *coords, lnh_stream_t stream);
/* Replaces packbits              raymarching.h:22-25 (raymarching.cu:286-319): N bytes from 8N floats. */
LNH_API int lnh_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, lnh_stream_t stream);
/* Cell index / occupancy bit of arbitrary points (the lookup inside kernel_march_rays_train,
 * raymarching.cu:386-408) — exposes the bit-exact indexing contract on its own. */
LNH_API int lnh_occupancy_lookup(const float *xyz, const float *dt, const uint8_t *bitfield, float bound, uint32_t N,
                                 uint32_t C, uint32_t H, uint32_t *cell_index, uint8_t *occ, lnh_stream_t stream);
/* Replaces march_rays_train      raymarching.h:27-44 (raymarching.cu:331-568).  counter [2] int32 zeroed by the
 * caller: [0] += points, [1] += rays; rays [N,3] = (ray id, offset, count) in atomic-allocation order. */
LNH_API int lnh_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound,
                                 float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                                 const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                                 int32_t *rays, int32_t *counter, const float *noises, lnh_stream_t stream);
/* Adds (no reference counterpart: the reference's marcher hands out rows with one pair of atomics per ray, in arrival order)
 * the RAY-ORDERED form of lnh_march_rays_train — same arguments, same refusals, no allocation, no synchronisation, N == 0
 * returns LNH_OK.  rays[n] = (n, sum of count_m over m < n, count_n) for every n; counter [2] int32 zeroed by the caller:
 * [0] += points, [1] += rays (the values lnh_march_rays_train leaves).  A ray with offset + count > M keeps its table entry
 * and writes no sample (its rows stay as the caller cleared them): with ordered offsets that set depends on the inputs
 * alone.  Per ray the samples are bit for bit lnh_march_rays_train's; the whole output equals the serial oracle's
 * (oracle/lnh_oracle.c).  Three launches on `stream` (count per ray, one-workgroup integer scan, write per ray); no
 * workgroup waits for another one, no float atomics. */
LNH_API int lnh_march_rays_train_ordered(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound,
                                         float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                                         uint32_t M, const float *nears, const float *fars, float *xyzs, float *dirs,
                                         float *deltas, int32_t *rays, int32_t *counter, const float *noises,
                                         lnh_stream_t stream);
/* Replaces composite_rays_train_forward / _backward  raymarching.h:45-69 (raymarching.cu:577-802). */
LNH_API int lnh_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                             const int32_t *rays, uint32_t M, uint32_t N, float T_thresh,
                                             float *weights_sum, float *depth, float *image, lnh_stream_t stream);
LNH_API int lnh_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image,
                                              const float *sigmas, const float *rgbs, const float *deltas,
                                              const int32_t *rays, const float *weights_sum, const float *image,
                                              uint32_t M, uint32_t N, float T_thresh, float *grad_sigmas,
                                              float *grad_rgbs, lnh_stream_t stream);
/*
 * LiDAR variant of the ragged compositing (no reference counterpart: the reference composites LiDAR rays with PyTorch
 * ops on dense [N,T] tensors, renderer.py:233-271, and its CUDA template above has 3 colour channels and no depth
 * gradient, raymarching.py:330).  feats [M,K] (K <= 3; K = 2: ray-drop, intensity), deltas [M,2] and xyzs [M,3] as
 * written by lnh_march_rays_train; depth = sum w * z with z = (xyz - o) . d the ABSOLUTE distance along the unit ray.
 * Backward: grad_sigmas [M] / grad_feats [M,K] ZERO-INITIALISED by the caller, includes the depth term.
 */
LNH_API int lnh_lidar_composite_rays_train_forward(const float *sigmas, const float *feats, const float *deltas,
                                                   const float *xyzs, const float *rays_o, const float *rays_d,
                                                   const int32_t *rays, uint32_t M, uint32_t N, uint32_t K,
                                                   float T_thresh, float *weights_sum, float *depth, float *image,
                                                   lnh_stream_t stream);
LNH_API int lnh_lidar_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_depth,
                                                    const float *grad_image, const float *sigmas, const float *feats,
                                                    const float *deltas, const float *xyzs, const float *rays_o,
                                                    const float *rays_d, const int32_t *rays,
                                                    const float *weights_sum, const float *depth, const float *image,
                                                    uint32_t M, uint32_t N, uint32_t K, float T_thresh,
                                                    float *grad_sigmas, float *grad_feats, lnh_stream_t stream);

/*
 * Inference variants (raymarching.h:55-69 march_rays / composite_rays; raymarching.cu:808-928, 966-1053): march the
 * first n_alive rays listed in rays_alive for at most n_step occupied samples from their current rays_t (outputs
 * [n_alive*n_step, 3|3|2], caller-zeroed: delta == 0 ends a ray), then accumulate sigmas / rgbs [n_alive*n_step, 1|3]
 * into weights_sum / depth / image [N, 1|1|3] in place; finished rays get rays_alive[n] = -1, the others their new t.
 */
LNH_API int lnh_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t,
                           const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                           uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars,
                           float *xyzs, float *dirs, float *deltas, const float *noises, lnh_stream_t stream);
LNH_API int lnh_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                               const float *sigmas, const float *rgbs, const float *deltas, float *weights_sum,
                               float *depth, float *image, lnh_stream_t stream);

/*
 * Alive-ray evaluation of LiDAR rays (NeRFRenderer.run_cuda_alive): one round = lnh_lidar_march_rays, the field on the
 * round's samples, lnh_lidar_composite_rays, lnh_alive_compact; repeat until no ray is alive.  The loop is the one of
 * march_rays / composite_rays above (raymarching.cu:808-928, 966-1053; raymarching.py:362-512); the sample lattice is the
 * one of lnh_march_rays_train (raymarching.cu:379-439), the compositing the one of lnh_lidar_composite_rays_train_forward.
 * No entry point here touches MLP element types: the same three serve the fp16 and the bf16 build of the field (no _bf16
 * twins); the field itself is the existing ragged chain (lnh_ragged_points, lnh_grid_encode_forward,
 * lnh_density_mlp_forward[_bf16], lnh_ragged_color_forward[_bf16]) on the table lnh_lidar_march_rays writes.
 *
 * State, all caller-allocated, N = rays of the call:
 *   rays_alive [N] int32 x 2, alive_count [1] int32 x 2   ping-pong halves: ray ids of the alive rays in slot order and
 *                                     how many.  The caller starts with 0 .. N-1 / N.  Every kernel clips the count to
 *                                     n_alive_max, the HOST's upper bound, which sizes launches and sample buffers.
 *   rays_t [N] f32                    resume parameter; the caller starts it at the ray's near.  lnh_lidar_march_rays
 *                                     stores the exact t behind the ray's last sample when the ray got all n_step samples
 *                                     of the round, else +inf = "left the box" (the walk passed far, or the ray holds its
 *                                     max_steps samples): t < far never holds again.
 *   rays_steps [N] int32              samples so far, ZEROED by the caller (the lattice walk emits at most max_steps per
 *                                     ray, raymarching.cu:436, over all rounds together).
 *   weights_sum [N], depth [N], image [N,K] f32   ZEROED by the caller;  transmittance [N] f32 set to ONE by the caller.
 *
 * lnh_lidar_march_rays: slot n < min(alive_count[0], n_alive_max) marches ray rays_alive[n] for at most n_step occupied
 * samples into rows [n * n_step, (n + 1) * n_step) of xyzs [n_alive_max * n_step, 3] / deltas [.., 2] (no clearing needed:
 * deltas of the rows a slot does not fill are written as 0, the end-of-ray mark of raymarching.cu:1003; their xyzs keep
 * whatever finite values they held) and writes ALL N rows of rays [N,3] = (ray id, first row, count) — (0, 0, 0) beyond
 * the alive count — the table the ragged field kernels and lnh_lidar_composite_rays walk.  Concatenated over the rounds,
 * a ray's xyzs / deltas are bit for bit the samples lnh_march_rays_train emits for it with noises = 0, whatever the
 * sequence of n_step.  samples_total (NULL or [1] int32, caller-zeroed) += samples of the round (integer atomic).
 *
 * lnh_lidar_composite_rays: sigmas [rows] (density_scale applied), feats [rows, K], K <= 3:
 *   alpha = 1 - exp(-sigma dt),  w = alpha T,  weights_sum += w,  depth += w ((xyz - o) . d),  image += w feat,
 *   T *= 1 - alpha, stop AFTER the sample that takes T below T_thresh (renderer.py:233-271 on ragged samples; the carried
 *   T, not the template's 1 - weights_sum).  A ray is dead — rays_alive[n] = -1 — when it stopped, when its round came back
 *   short of n_step samples, or when rays_t holds the mark.  One group of min(64, n_step rounded up to a power of two) lanes
 *   per ray, one lane per sample.
 *
 * lnh_alive_compact: the entries >= 0 of rays_alive[0 .. min(alive_count[0], n_alive_max)), in slot order, to
 * rays_alive_out; their number to alive_count_out[0].  One workgroup; the order never depends on timing.
 */
LNH_API int lnh_lidar_march_rays(uint32_t n_alive_max, uint32_t n_step, uint32_t N, const int32_t *alive_count,
                                 const int32_t *rays_alive, float *rays_t, int32_t *rays_steps, const float *rays_o,
                                 const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                                 uint32_t max_steps, uint32_t C, uint32_t H, const float *fars, float *xyzs,
                                 float *deltas, int32_t *rays, int32_t *samples_total, lnh_stream_t stream);
LNH_API int lnh_lidar_composite_rays(uint32_t n_alive_max, uint32_t n_step, uint32_t N, uint32_t K, float T_thresh,
                                     const int32_t *alive_count, int32_t *rays_alive, const float *rays_t,
                                     const int32_t *rays, const float *sigmas, const float *feats, const float *deltas,
                                     const float *xyzs, const float *rays_o, const float *rays_d, float *weights_sum,
                                     float *depth, float *image, float *transmittance, lnh_stream_t stream);
LNH_API int lnh_alive_compact(uint32_t n_alive_max, const int32_t *alive_count, const int32_t *rays_alive,
                              int32_t *rays_alive_out, int32_t *alive_count_out, lnh_stream_t stream);

/* ------------------------------------------------------------------ LiDAR renderer kernels ------------------ */
/*
 * The reference composites LiDAR rays with ~40 PyTorch launches (lidarnerf/nerf/renderer.py:180-271).  These
 * entry points are the same arithmetic as single kernels, one 64-lane wavefront per ray.
 *
 * lnh_lidar_weights: renderer.py:233-243 (and 180-194).  z [N,T] sorted per ray, sigma [N,T], sample_dist [N];
 *   deltas_i = z_{i+1}-z_i (last = sample_dist), alpha = 1-exp(-delta*density_scale*sigma),
 *   w = alpha * prod_{j<i}(1-alpha_j+1e-15).  Writes weights [N,T] f32.
 */
LNH_API int lnh_lidar_weights(const float *z, const float *sigma, const float *sample_dist, uint32_t N, uint32_t T,
                              float density_scale, float *weights, lnh_stream_t stream);
/*
 * lnh_lidar_composite_forward: renderer.py:233-271.  rgb [N,T,K] f32 (already zero where weights <= 1e-4,
 * network.py:204-208).  Outputs weights [N,T], weights_sum [N], depth [N] = sum w*z, image [N,K] = sum w*rgb.
 */
LNH_API int lnh_lidar_composite_forward(const float *z, const float *sigma, const float *rgb,
                                        const float *sample_dist, uint32_t N, uint32_t T, uint32_t K,
                                        float density_scale, float *weights, float *weights_sum, float *depth,
                                        float *image, lnh_stream_t stream);
/*
 * lnh_lidar_composite_backward: exact adjoint of the PyTorch graph above (autograd of cumprod / exp / sums),
 * INCLUDING the depth gradient (the reference's CUDA composite drops it, raymarching.py:330; the LiDAR loss is
 * depth dominated so the PyTorch path is the one to follow).  grad_* of the three outputs -> grad_sigma [N,T],
 * grad_rgb [N,T,K].
 */
LNH_API int lnh_lidar_composite_backward(const float *grad_weights_sum, const float *grad_depth,
                                         const float *grad_image, const float *z, const float *sigma,
                                         const float *rgb, const float *sample_dist, uint32_t N, uint32_t T,
                                         uint32_t K, float density_scale, float *grad_sigma, float *grad_rgb,
                                         lnh_stream_t stream);
/*
 * lnh_lidar_resample: renderer.py:180-231 in one kernel — stage-1 weights, sample_pdf (renderer.py:10-46) with
 * the caller's uniforms u [N,n_new] (linspace for det, rand for training), then the sort/merge of the old and new
 * z values.  Outputs new_z [N,n_new] (sorted_new = 0: in sample_pdf's order, exactly what the reference hands to
 * its second density query; sorted_new = 1: ascending, same set of values), merged z_out [N,T+n_new] ascending
 * and perm [N,T+n_new] int32: the position in concat([old, new]) each merged element came from (= torch.sort's
 * index, renderer.py:218).
 */
LNH_API int lnh_lidar_resample(const float *z, const float *sigma, const float *sample_dist, const float *u,
                               uint32_t N, uint32_t T, uint32_t n_new, float density_scale, uint32_t sorted_new,
                               float *new_z, float *z_out, int32_t *perm, lnh_stream_t stream);
/* The same with the rows of `sigma` sigma_stride (>= T) floats apart: the fused render step keeps the coarse and the
 * importance samples of a ray side by side in one [N, T+n_new] buffer and resamples from its first T columns. */
LNH_API int lnh_lidar_resample_strided(const float *z, const float *sigma, uint32_t sigma_stride,
                                       const float *sample_dist, const float *u, uint32_t N, uint32_t T,
                                       uint32_t n_new, float density_scale, uint32_t sorted_new, float *new_z,
                                       float *z_out, int32_t *perm, lnh_stream_t stream);
/* lnh_lidar_resample_strided with sorted_new = 1 that also writes the grid coordinates of the new samples
 * (lnh_lidar_sample_points for slots T .. T+n_new-1) into x01 [N*(T+n_new), 3]: the importance pass of the fused step
 * needs no separate coordinate kernel. */
LNH_API int lnh_lidar_resample_points(const float *z, const float *sigma, uint32_t sigma_stride,
                                      const float *sample_dist, const float *u, uint32_t N, uint32_t T, uint32_t n_new,
                                      float density_scale, float *new_z, float *z_out, int32_t *perm,
                                      const float *rays_o, const float *rays_d, const float *aabb, float bound,
                                      float *x01, lnh_stream_t stream);


/* ------------------------------------------------------------------ fused LiDAR field step ------------------ */
/*
 * The kernels below fuse what lidarnerf/nerf/renderer.py:149-256 + lidarnerf/nerf/network.py:162-237 spread over
 * dozens of PyTorch launches (sample positions, encoder permutes, trunc_exp, sort/gather merge, masked colour
 * query).  Semantics are unchanged; see lidar-nerf_amd/csrc/lidar_field.hip for the derivations.
 *
 * lnh_lidar_sample_points: (clip(o + d*z, aabb) + bound) / (2 bound)  (renderer.py:164-167, grid.py:213) for z [N,T],
 * written to row n*T_tot + slot_off + j of x01 (T_tot = T, slot_off = 0: plain [N*T,3]).
 */
LNH_API int lnh_lidar_sample_points(const float *rays_o, const float *rays_d, const float *z, const float *aabb,
                                    float bound, uint32_t N, uint32_t T, uint32_t T_tot, uint32_t slot_off, float *x01,
                                    lnh_stream_t stream);
/* lnh_lidar_coarse_samples (below: the stratified depths of renderer.py:140-156, u = NULL for the unperturbed ones) and
 * lnh_lidar_sample_points of those depths (slot_off = 0) in one launch; z [N,T] and x01 rows n*T_tot + j are written. */
LNH_API int lnh_lidar_coarse_sample_points(const float *u, const float *rays_o, const float *rays_d, const float *aabb,
                                           float bound, uint32_t N, uint32_t T, uint32_t T_tot, float near, float far,
                                           float *z, float *x01, lnh_stream_t stream);
/*
 * lnh_grid_encode_forward_mapped: lnh_grid_encode_forward (D = 3, hash, linear) whose launch index b = r*T_cur + j
 * reads position row r*T_tot + slot_off + j of inputs_all [B_all,3] and writes the same row of
 * outputs_all [L, B_all, C] — coarse and importance samples of a ray share one buffer, so the backward pass is ONE
 * launch over B_all points.
 */
LNH_API int lnh_grid_encode_forward_mapped(const float *inputs_all, const void *embeddings, const int32_t *offsets_host,
                                           void *outputs_all, uint32_t B, uint32_t T_cur, uint32_t T_tot,
                                           uint32_t slot_off, uint32_t B_all, uint32_t C, uint32_t L, float S,
                                           uint32_t H, int dtype, lnh_stream_t stream);
/* lnh_grid_encode_forward_mapped with a gridtype: 0 (hash) or 2 (tiny-cuda-nn lattice); the entry point above is this one
 * with gridtype 0.  (lnh_version >= 101) */
LNH_API int lnh_grid_encode_forward_mapped_ex(const float *inputs_all, const void *embeddings, const int32_t *offsets_host,
                                              void *outputs_all, uint32_t B, uint32_t T_cur, uint32_t T_tot,
                                              uint32_t slot_off, uint32_t B_all, uint32_t C, uint32_t L, float S,
                                              uint32_t H, uint32_t gridtype, int dtype, lnh_stream_t stream);
/*
 * lnh_density_mlp_forward: sigma-net 32 -> 64 -> 16 (ReLU, no bias; network.py:45-59,162-179) on features in the
 * encoder's level-major layout [16,B,2] (fp16).  Point p = r*T_cur + j writes row r*T_tot + slot_off + j of
 * h16 [*,16] fp16 (raw outputs: col 0 density pre-activation, cols 1..15 geo_feat) and sigma [*] f32 = exp(h16[.,0])
 * (trunc_exp forward).  weights flat fp16 [64*32 | 16*64].  feat_rows = 0: features is [16,B,2] indexed by p;
 * feat_rows = B_all: features is [16,B_all,2] indexed by the destination row (lnh_grid_encode_forward_mapped).
 */
LNH_API int lnh_density_mlp_forward(const void *features, const void *weights, uint32_t B, uint32_t T_cur,
                                    uint32_t T_tot, uint32_t slot_off, uint32_t feat_rows, void *h16, float *sigma,
                                    lnh_stream_t stream);
/* grad_h16 rows addressed like h16 above -> grad_features [16,B,2] fp16, grad_weights fp32 += (fixed-order sum, see
 * lnh_wgrad_workspace_bytes). */
LNH_API int lnh_density_mlp_backward(const void *grad_h16, const void *features, const void *weights, uint32_t B,
                                     uint32_t T_cur, uint32_t T_tot, uint32_t slot_off, void *grad_features,
                                     float *grad_weights, void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
/*
 * lnh_lidar_merge_weights: sigma_m[n,i] = sigma_pt[n, perm[n,i]] and the compositing weights of the merged samples
 * (renderer.py:217-243); z [N,T] merged (sorted) depths, perm from lnh_lidar_resample.
 */
LNH_API int lnh_lidar_merge_weights(const float *z, const float *sigma_pt, const int32_t *perm,
                                    const float *sample_dist, uint32_t N, uint32_t T, float density_scale,
                                    float *sigma_m, float *weights, lnh_stream_t stream);
/*
 * Element-wise stages around the field that the reference leaves to dozens of PyTorch launches (one launch each here).
 * lnh_lidar_coarse_samples: z[n,i] = near + (far-near)*linspace(0,1,T)[i] (+ (u[n,i]-0.5)*(far-near)/T when u != NULL)
 *   (renderer.py:147-161; linspace evaluated symmetrically like torch.linspace).
 * lnh_lidar_dir_term: per-ray direction term of the colour head's first Linear (network.py:215-221):
 *   features16[n,k] = fp16-rounded dir_features[n,k] (kept as f32), cdir[n,o] = sum_k features16[n,k]*fp16(w0[o*ldw+k]),
 *   o < 64, K <= 128.
 * lnh_lidar_pack_weights: fp32 master matrices (row strides ld_*) -> flat fp16 vectors of lnh_density_mlp_* (wsig16:
 *   [64,32 | 16,64]) and lnh_lidar_color_* (wcol16: W0g [64,16] = (0 | wc0[:, n_dir:n_dir+15]) | wc1 [64,64] | wc2 -> [16,64]).
 * lnh_lidar_loss: nerf/utils.py:712-746 default criteria, loss = mean_n(alpha_d*|d-gd| + alpha_r*(r-gr)^2 +
 *   alpha_i*(i-gi)^2) with predictions/targets masked by gt ray-drop; gt [N,3] = (raydrop, intensity, depth); also
 *   writes d loss/d depth [N] and d loss/d image [N,2], multiplied by *grad_scale when grad_scale != NULL (the loss
 *   scale of the training step: backward() then has nothing left to multiply).  `loss` need not be cleared.
 *   grad_depth / grad_image may be NULL (each on its own): that gradient is not written — the value alone, for a step whose
 *   gradients lnh_lidar_color_composite_forward_train has formed.
 */
LNH_API int lnh_lidar_coarse_samples(const float *u, uint32_t N, uint32_t T, float near, float far, float *z,
                                     lnh_stream_t stream);
LNH_API int lnh_lidar_dir_term(const float *dir_features, const float *w0, uint32_t ldw, uint32_t N, uint32_t K,
                               float *features16, float *cdir, lnh_stream_t stream);
/* The same with the frequency encoder of the directions folded in: dirs [N,3] -> features [N, 3 + 6*degree]
 * (lnh_freq_encode_forward's layout and arithmetic: x | sin(2^f x), sin(2^f x + pi/2) per band) -> features16, cdir. */
LNH_API int lnh_lidar_dir_term_freq(const float *dirs, uint32_t degree, const float *w0, uint32_t ldw, uint32_t N,
                                    float *features16, float *cdir, lnh_stream_t stream);
/* grad_w0[o*ldw + k] += sum_n ray_sum[n,o] * features16[n,k], k < K  (ray_sum [N,64] from lnh_lidar_color_backward; the
 * sum over the rays is formed in a fixed order — wgrad_ws, see lnh_wgrad_workspace_bytes — and ADDED: clear grad_w0 first).  grad_w0g != NULL: the packed [64,16] gradient of the colour
 * head's geo-feature columns (what lnh_lidar_color_backward accumulates at the front of its grad_w) is copied to
 * grad_w0[o*ldw + K + c] = grad_w0g[o*16 + 1 + c], c < 15 — the whole gradient of network.py:199's first Linear in one launch. */
LNH_API int lnh_lidar_dir_term_backward(const float *ray_sum, const float *features16, uint32_t N, uint32_t K,
                                        const float *grad_w0g, float *grad_w0, uint32_t ldw, void *wgrad_ws,
                                        uint64_t wgrad_ws_bytes, lnh_stream_t stream);
LNH_API int lnh_lidar_pack_weights(const float *ws0, uint32_t ld_s0, const float *ws1, uint32_t ld_s1,
                                   const float *wc0, uint32_t ld_c0, uint32_t n_dir, const float *wc1, uint32_t ld_c1,
                                   const float *wc2, uint32_t ld_c2, void *wsig16, void *wcol16, lnh_stream_t stream);
/* Everything a fused render step needs before its first encode, in ONE launch: lnh_lidar_pack_weights (n_dir = 3 + 6 *
 * degree) + lnh_lidar_dir_term_freq (on rays_d, against wc0) + lnh_lidar_coarse_sample_points — the same arithmetic, bit
 * for bit (renderer.py:129-167 sampling set-up, network.py:215-221 direction term). */
LNH_API int lnh_lidar_step_prologue(const float *ws0, uint32_t ld_s0, const float *ws1, uint32_t ld_s1, const float *wc0,
                                    uint32_t ld_c0, uint32_t degree, const float *wc1, uint32_t ld_c1, const float *wc2,
                                    uint32_t ld_c2, void *wsig16, void *wcol16, const float *u, const float *rays_o,
                                    const float *rays_d, const float *aabb, float bound, uint32_t N, uint32_t T,
                                    uint32_t T_tot, float near, float far, float *z, float *x01, float *features16,
                                    float *cdir, lnh_stream_t stream);
LNH_API int lnh_lidar_loss(const float *depth, const float *image, const float *gt, uint32_t N, float alpha_d,
                           float alpha_r, float alpha_i, const float *grad_scale, float *loss, float *grad_depth,
                           float *grad_image, lnh_stream_t stream);
/* The same with the structural-gradient term of the reference's patch epochs (nerf/utils.py:760-876, non-sobel grad_loss):
 * rays come as N / (px * py) patches of px x py pixels, row-major; + alpha_grad * mean_{patch, row, j < py-1} |
 * |pd_j - pd_j+1| m_j - (gd_j - gd_j+1) m_j |, depths in metres (value / scale), m_j = raydrop_j * (|gd_j - gd_j+1| < 0.01). */
LNH_API int lnh_lidar_loss_patch(const float *depth, const float *image, const float *gt, uint32_t N, uint32_t px,
                                 uint32_t py, float scale, float alpha_d, float alpha_r, float alpha_i, float alpha_grad,
                                 const float *grad_scale, float *loss, float *grad_depth, float *grad_image,
                                 lnh_stream_t stream);
/*
 * lnh_lidar_loss_ex (lnh_version >= 102): the reference's Trainer.train_step loss (nerf/utils.py:697-884) for ANY option
 * set of its CLI (main_lidarnerf.py:46-60, 92-103, 330-342), with the contract of lnh_lidar_loss_patch: writes *loss and
 * d loss/d depth [N], d loss/d image [N,2], the gradients multiplied by *grad_scale when grad_scale != NULL.
 * Criterion codes (LNH_LOSS_*): L1, MSE, HUBER (torch.nn.HuberLoss, delta = huber_delta; the CLI's is 0.2 * scale) and BCE
 * (BCEWithLogitsLoss on the prediction as given: (1 - y) x - log sigmoid(x)) in every slot, COS in the grad slot only.
 * Semantics, term for term the reference's:
 *   - per ray: alpha_d C_depth(d gr, gd gr) + alpha_r C_raydrop(r, gr) + alpha_i C_intensity(i gr, gi gr), mean over N;
 *     predictions and targets masked by the ground-truth ray-drop gr before every criterion.
 *   - px > 1 (patch epochs; rays are N / (px py) patches of px x py pixels, row-major): depths in metres (value / scale).
 *     Without LNH_LOSS_SOBEL the prediction gradient is |neighbour difference| (x: along py, [px, py-1]; y: along px,
 *     [px-1, py]); with it, the SIGNED 3x3 Sobel responses with zero padding inside each patch ([px, py] each).
 *     dx = |grad x|, dy = |grad y|.  GRAD_NORM_SMOOTH: + alpha_grad_norm (mean e^-dx + mean e^-dy); SPATIAL:
 *     + alpha_spatial (mean dx^2 + mean dy^2); TV: + alpha_tv (mean dx + mean dy) — each mean over its own tensor.
 *   - LNH_LOSS_GRAD: + alpha_grad * mean C_grad(grad x * m, gt grad x * m), only the x term; m = gr * (|gt grad x| < 0.01),
 *     cropped to [px, py-1] without Sobel (gr of the left pixel), full size with it.  COS: 1 - CosineSimilarity per patch
 *     over the flattened masked vectors, mean over the patches, with torch's eps handling (torch 2.x):
 *     cos = u.w / (max(|u|, 1e-8) max(|w|, 1e-8)), d cos/du = w / (max(|u|,eps) max(|w|,eps)) - cos u / (max(|u|,eps) |u|)
 *     (the clamp is invisible to autograd; the second term is 0 at |u| = 0): an all-zero patch gives cos 0, gradient 0.
 *   - d|x|/dx at 0 is 0 (torch's sign).
 * Deterministic (fixed-order sums, no atomics) and stateless.  workspace: lnh_lidar_loss_ex_workspace_bytes(N) bytes of
 * device scratch, 4-byte aligned, contents irrelevant (per-workgroup partial sums; a second launch adds them in order).
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null pointer, an unknown criterion code or COS outside the grad
 * slot, N % (px py) != 0, px > 1 with py < 2, scale <= 0 on patch epochs, a workspace smaller than the query.
 */
enum { LNH_LOSS_L1 = 0, LNH_LOSS_MSE = 1, LNH_LOSS_HUBER = 2, LNH_LOSS_BCE = 3, LNH_LOSS_COS = 4 };
enum {
    LNH_LOSS_SOBEL = 1, LNH_LOSS_GRAD = 2, LNH_LOSS_GRAD_NORM_SMOOTH = 4, LNH_LOSS_SPATIAL = 8, LNH_LOSS_TV = 16
};
typedef struct lnh_lidar_loss_options {
    int32_t depth_loss, raydrop_loss, intensity_loss, grad_loss; /* LNH_LOSS_L1 .. LNH_LOSS_COS */
    uint32_t flags;                                              /* LNH_LOSS_SOBEL | LNH_LOSS_GRAD | ... */
    uint32_t px, py;                                             /* patch shape; px <= 1: per-ray terms only */
    float scale, huber_delta;
    float alpha_d, alpha_r, alpha_i, alpha_grad, alpha_grad_norm, alpha_spatial, alpha_tv;
} lnh_lidar_loss_options;
LNH_API uint64_t lnh_lidar_loss_ex_workspace_bytes(uint32_t N);
LNH_API int lnh_lidar_loss_ex(const float *depth, const float *image, const float *gt, uint32_t N,
                              const lnh_lidar_loss_options *options, const float *grad_scale, void *workspace,
                              uint64_t workspace_bytes, float *loss, float *grad_depth, float *grad_image,
                              lnh_stream_t stream);
/*
 * The LiDAR colour head on the marcher's RAGGED samples (BASELINE config 4; network.py:199-237 evaluated on the samples of
 * renderer.run_cuda, which the reference dropped while keeping raymarching.cu:331-772), with the dense chain's two moves:
 * the direction part of the first Linear once per RAY (cdir [N,64] from lnh_lidar_dir_term_freq on rays_d) and the
 * sample's sigma-net row as the 16-wide input.  rays [N,3] i32 = the marcher's table (ray index, first sample, count);
 * a ray whose samples do not fit M has none.  w16 = lnh_lidar_pack_weights' wcol16.
 * lnh_ragged_color_forward: rgb[m] = sigmoid(head(h16[m], cdir[ray])) [M,2] for every owned sample (others untouched).
 * lnh_ragged_color_backward: grad_h16 rows of the owned samples (col 0 = grad_sigma * density_scale * exp(clamp(h0)), cols
 *   1..15 through the head; rows nobody owns are NOT written: clear grad_h16 first), grad_w += (layout of wcol16, fp32),
 *   ray_sum [N,64] = sum over the ray's samples of d(first hidden pre-activation), indexed by ray INDEX (feeds
 *   lnh_lidar_dir_term_backward; rows of rays without an entry are not written).
 */
LNH_API int lnh_ragged_color_forward(const void *h16, const int32_t *rays, const float *cdir, const void *w16, uint32_t N,
                                     uint32_t M, float *rgb, lnh_stream_t stream);
LNH_API int lnh_ragged_color_backward(const float *grad_rgb, const float *grad_sigma, float density_scale, const void *h16,
                                      const int32_t *rays, const float *cdir, const void *w16, uint32_t N, uint32_t M,
                                      void *grad_h16, float *grad_w, float *ray_sum, void *wgrad_ws,
                                      uint64_t wgrad_ws_bytes, lnh_stream_t stream);
/*
 * Element-wise stages of the occupancy-grid render chain over the marcher's flat sample list [M] (BASELINE config 4; the
 * reference kept torch-ngp's kernels, raymarching.cu:331-772, and dropped this caller — what runs between them are the
 * tensor expressions of network.py:162-237 on [M, *] tensors: one launch each here).
 * lnh_ragged_points: x01 = (xyz + bound) / (2 bound) (gridencoder/grid.py:213).
 * lnh_ragged_pack_weights: fp32 master matrices -> wsig16 [64,32 | 16,64] and wcol16 [64,96 (wc0[:, :n_in], zero-padded) |
 *   64,64 | 16,64 (wc2 in rows 0..1)] — the flat vectors of lnh_density_mlp_* / lnh_mlp_*(input_dim 96, one hidden matrix).
 * lnh_ragged_color_input: cin [M,96] = [x | sin(2^f x), sin(2^f x + pi/2), f < degree (freqencoder.cu:34-63) of the
 *   sample's direction | geo_feat = h16[m, 1:16] | 0] (network.py:215-221), in the MLP element type.
 * lnh_ragged_color_input_rays: the same rows written ray by ray from the marcher's rays [N,3] (id, offset, count): a
 *   ray's samples share its direction (raymarching.cu:331-534), so the direction terms are evaluated once per ray from
 *   dirs[offset]; rows no ray owns (deltas[m,0] == 0: the unused tail, the slots of a ray dropped for lack of room) are
 *   set to zero.  Same values as lnh_ragged_color_input on the rows rays own.
 * lnh_ragged_color_output: rgb [M,2] f32 = sigmoid(y16[m, 0:2]) (network.py:224).  _backward: grad_y16 [M,16] =
 *   (grad_rgb * rgb * (1 - rgb) | 0).
 * lnh_ragged_grad_rows: grad_h16[m,0] = grad_sigma[m] * density_scale * exp(clamp(h16[m,0], -15, 15)) (trunc_exp backward,
 *   activation.py:17-19), grad_h16[m,1:16] = grad_cin[m, n_dir : n_dir + 15], n_dir = 3 + 6 * degree.
 */
LNH_API int lnh_ragged_points(const float *xyz, float bound, uint32_t M, float *x01, lnh_stream_t stream);
LNH_API int lnh_ragged_pack_weights(const float *ws0, uint32_t ld_s0, const float *ws1, uint32_t ld_s1, const float *wc0,
                                    uint32_t ld_c0, uint32_t n_in, const float *wc1, uint32_t ld_c1, const float *wc2,
                                    uint32_t ld_c2, void *wsig16, void *wcol16, lnh_stream_t stream);
LNH_API int lnh_ragged_color_input(const float *dirs, const void *h16, uint32_t M, uint32_t degree, void *cin,
                                   lnh_stream_t stream);
LNH_API int lnh_ragged_color_input_rays(const float *dirs, const void *h16, const int32_t *rays, const float *deltas,
                                        uint32_t N, uint32_t M, uint32_t degree, void *cin, lnh_stream_t stream);
LNH_API int lnh_ragged_color_output(const void *y16, uint32_t M, float *rgb, lnh_stream_t stream);
LNH_API int lnh_ragged_color_output_backward(const float *grad_rgb, const float *rgb, uint32_t M, void *grad_y16,
                                             lnh_stream_t stream);
LNH_API int lnh_ragged_grad_rows(const float *grad_sigma, float density_scale, const void *h16, const void *grad_cin,
                                 uint32_t degree, uint32_t M, void *grad_h16, lnh_stream_t stream);
/*
 * lnh_lidar_color_forward: LiDAR colour head (network.py:199-237 with cal_lidar_color=True) on merged samples:
 * rgb[n,i,0:2] = sigmoid(MLP([freq(d_n) | geo_feat(sample)])) where weights[n,i] > 1e-4, else 0.
 * h16 [N*T,16] sigma-net rows in point order, perm [N,T], cdir [N,64] f32 = W0[:, :75] freq(d_n) (per ray),
 * w16 flat fp16: W0g [64,16] (col 0 zero, cols 1..15 = W0[:,75:90]) | W1 [64,64] | W2 padded to [16,64].
 */
LNH_API int lnh_lidar_color_forward(const void *h16, const int32_t *perm, const float *weights, const float *cdir,
                                    const void *w16, uint32_t N, uint32_t T, float *rgb, lnh_stream_t stream);
/*
 * lnh_lidar_color_composite_forward: the forward tail of the fused render step in one launch, one wave per ray —
 * lnh_lidar_merge_weights (renderer.py:217-243) + lnh_lidar_color_forward + lnh_lidar_composite_forward
 * (renderer.py:233-271) with the weights and the merge permutation of a ray kept in LDS in between.  Inputs as for those
 * three (z [N,T] merged depths, sigma_pt [N,T] point order, perm from lnh_lidar_resample); outputs sigma_m, weights
 * [N,T], rgb [N,T,2], weights_sum, depth [N], image [N,2].  sigma_m, weights, weights_sum and depth are bit-identical
 * to the separate entry points, image to fp32 rounding (different summation order).  T <= 2048.
 */
LNH_API int lnh_lidar_color_composite_forward(const float *z, const float *sigma_pt, const int32_t *perm,
                                              const float *sample_dist, const void *h16, const float *cdir,
                                              const void *w16, uint32_t N, uint32_t T, float density_scale,
                                              float *sigma_m, float *weights, float *rgb, float *weights_sum,
                                              float *depth, float *image, lnh_stream_t stream);
/*
 * lnh_lidar_color_composite_forward_train: the same forward tail for a TRAINING step under the default loss (nerf/utils.py:
 * 712-746 = lnh_lidar_loss, one ray per patch) — weights, weights_sum, depth and image of lnh_lidar_color_composite_forward
 * with the same bits (sigma_m and rgb, which only the compositing backward read, stay in the workgroup's LDS and are NOT
 * written), and then, in the wave that has just finished the ray n:
 *   grad_image[n,:], d loss / d depth[n] — lnh_lidar_loss's gradients of that ray (a closed form of depth[n], image[n,:],
 *     gt[n,:] = (raydrop, intensity, depth), N and the three alphas; times *grad_scale when grad_scale != NULL; sign(0) = 0),
 *   grad_sigma[n,:] — lnh_lidar_composite_backward (K = 2, grad_weights_sum = NULL, grad_rgb = NULL) on those two, the
 *     adjoint of renderer.py:217-298's weights / depth / image,
 * both bit-identical to the chain lnh_lidar_color_composite_forward -> lnh_lidar_loss -> lnh_lidar_composite_backward (the
 * kernels share the per-ray loss and the two passes of the adjoint as device functions: same expressions, same lane <->
 * sample mapping, same summation order; the adjoint takes alpha_i and T_i as the forward walk of the same wave formed
 * them instead of walking the ray again).  The backward pass then starts at lnh_lidar_color_backward_image.  The loss
 * VALUE is not formed here: call lnh_lidar_loss on depth / image with grad_depth = grad_image = NULL.  T <= 2048.
 * (Added without moving lnh_version: detect by symbol.)
 */
LNH_API int lnh_lidar_color_composite_forward_train(const float *z, const float *sigma_pt, const int32_t *perm,
                                                    const float *sample_dist, const void *h16, const float *cdir,
                                                    const void *w16, uint32_t N, uint32_t T, float density_scale,
                                                    const float *gt, float alpha_d, float alpha_r, float alpha_i,
                                                    const float *grad_scale, float *weights, float *weights_sum,
                                                    float *depth, float *image, float *grad_sigma, float *grad_image,
                                                    lnh_stream_t stream);
/*
 * lnh_lidar_color_backward: grad_rgb [N,T,2], grad_sigma [N,T] (merged order, from lnh_lidar_composite_backward)
 * -> grad_h16 [N*T,16] fp16 in POINT order (col 0 = grad_sigma * exp(clamp(pre,-15,15)), activation.py:17-19;
 * cols 1..15 = colour-head input gradient), grad_w fp32 flat like w16 (+=, fixed-order sum: wgrad_ws), ray_sum [N,64] f32 = sum over
 * the ray of d(hidden0) (multiply by freq(d) to get the gradient of W0[:, :75]).
 */
LNH_API int lnh_lidar_color_backward(const float *grad_rgb, const float *grad_sigma, const void *h16,
                                     const int32_t *perm, const float *weights, const float *cdir, const void *w16,
                                     uint32_t N, uint32_t T, void *grad_h16, float *grad_w, float *ray_sum,
                                     void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
/* The same with grad_rgb formed on the fly from grad_image [N,2] = d loss / d image: grad_rgb[n,i,:] = weights[n,i] *
 * grad_image[n,:], which is all lnh_lidar_composite_backward would have written there (call it with grad_rgb = NULL):
 * the [N,T,2] gradient never travels through HBM. */
LNH_API int lnh_lidar_color_backward_image(const float *grad_image, const float *grad_sigma, const void *h16,
                                           const int32_t *perm, const float *weights, const float *cdir,
                                           const void *w16, uint32_t N, uint32_t T, void *grad_h16, float *grad_w,
                                           float *ray_sum, void *wgrad_ws, uint64_t wgrad_ws_bytes,
                                           lnh_stream_t stream);

/* ---- range image <-> point cloud (lidarnerf/convert.py:99-160, 194-237) ---------------------------
 * lnh_lidar_to_pano: points [N,4] f32 (x,y,z,intensity) in the sensor frame -> pano [H,W] f32 (distance of the nearest
 *   point per pixel, 0 = empty) and intensities [H,W] f32; lidar_K = (fov_up, fov) in degrees; points with
 *   dist >= max_depth or outside the image are dropped; ties keep the earlier point.  keys_scratch: H*W*8 bytes.
 * lnh_pano_to_lidar: pano (+ optional intensities) -> points [H*W,4] and valid [H*W] u8 (pano != 0); the caller
 *   compacts in pixel order.
 */
LNH_API int lnh_lidar_to_pano(const float *points, uint32_t N, uint32_t H, uint32_t W, float fov_up, float fov,
                              float max_depth, void *keys_scratch, float *pano, float *intensities,
                              lnh_stream_t stream);
LNH_API int lnh_pano_to_lidar(const float *pano, const float *intensities, uint32_t H, uint32_t W, float fov_up,
                              float fov, float *points, uint8_t *valid, lnh_stream_t stream);

/* ---- the two other projections of convert.py.  (Added without moving lnh_version: detect by symbol.)
 * Replaces lidar_to_pano_with_intensities_with_bbox_mask   lidarnerf/convert.py:4-97.
 * lnh_lidar_to_pano_masked: lnh_lidar_to_pano inside the window of rows [r0, r1) and columns [c0, c1) (0 <= r0 <= r1 <= H,
 *   0 <= c0 <= c1 <= W; the caller derives it from the projected box corners), with the intensity divided by max_intensity
 *   in float32; outside the window pano = -1 and intensities = 0.  keys_scratch: H*W*8 bytes.
 * Replaces lidar_to_pano_with_intensities_fpa + parse_z_buffer   lidarnerf/convert.py:253-361.
 * lnh_lidar_to_pano_fpa: "first-peak averaging".  A pixel that received n points (projection, max_depth and bounds tests of
 *   lnh_lidar_to_pano), with L = z_buffer_len:
 *     n == 0          (0, 0)
 *     n == 1          that point's (dist, intensity)
 *     2 <= n <= L     the points in point-index order WITHOUT the last-arrived one
 *     n > L           the L smallest under (dist, point index) WITHOUT the largest of them; L == 1: the smallest point itself
 *   of these, the ones with dist <= min dist + threshold (float64 on the float32 depths) give
 *   pano = sum(d w) / sum(w), intensities = sum(i w) / sum(w), w = 1 / d, in float64, stored as float32.
 *   The result depends on the order of the points in `points` (as the reference's does) and on nothing else: no float
 *   atomics, and the order in which threads arrive is never read.  1 <= z_buffer_len <= 32, H * W <= 2^24, N < 2^32
 *   (LNH_ERR_UNSUPPORTED otherwise).  workspace: lnh_lidar_to_pano_fpa_workspace_size(N, H, W) bytes, 8-byte aligned,
 *   contents irrelevant (0 for an unsupported shape).  The reference's threshold is 0.2.
 */
LNH_API int lnh_lidar_to_pano_masked(const float *points, uint32_t N, uint32_t H, uint32_t W, float fov_up, float fov,
                                     float max_depth, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1,
                                     float max_intensity, void *keys_scratch, float *pano, float *intensities,
                                     lnh_stream_t stream);
LNH_API uint64_t lnh_lidar_to_pano_fpa_workspace_size(uint64_t N, uint32_t H, uint32_t W);
LNH_API int lnh_lidar_to_pano_fpa(const float *points, uint64_t N, uint32_t H, uint32_t W, float fov_up, float fov,
                                  float max_depth, uint32_t z_buffer_len, double threshold, void *workspace,
                                  uint64_t workspace_bytes, float *pano, float *intensities, lnh_stream_t stream);

/* ---- mesh export: marching cubes over a density volume.  (Added without moving lnh_version: detect by symbol.)
 * Replaces extract_geometry / mcubes.marching_cubes, nerf/utils.py:169-184.
 * volume: fp32 [nx, ny, nz], z fastest (the reference's u[x, y, z]).  A corner is below iff v < iso (a value equal to iso and
 *   a NaN are not below); an edge crosses iff exactly one end is below.  The 256 cases are derived by csrc/gen_mc_tables.py
 *   (its own face rule and triangle order, not PyMCubes' table; the vertex set does not depend on the table).
 * lnh_marching_cubes_count: counts u32[4] (device) = vertices V, triangles T, non-finite samples of the volume, 0.  A count
 *   that does not fit 32 bits is stored as 0xffffffff.  Leaves in the workspace what lnh_marching_cubes_emit reads: call emit
 *   after it on the same stream with the same volume, sizes, iso and workspace.
 * lnh_marching_cubes_emit: vertices f32 [V,3] in index units (as mcubes returns them), triangles i32 [T,3]; never writes
 *   past max_vertices / max_triangles rows.  Order: a vertex belongs to the lattice point at the lower end of its edge;
 *   vertices in lattice-point order (flattened [x,y,z]), within a point its +x, +y, +z edge; a vertex shared by up to four
 *   cells appears once.  On an edge from value va to its +axis neighbour vb: t = (iso - va) / (vb - va), moving coordinate
 *   float(i) + t, in fp32.  Triangles in cell order (flattened [x,y,z] over (nx-1)(ny-1)(nz-1) cells), within a cell the
 *   table's; normals ((b - a) x (c - a)) point to the below side — on a density field, out of the dense matter.
 *   The mesh is a function of (volume, iso) alone: no atomics, and no workgroup waits for another.
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null pointer, a dimension below 2, a NaN iso, a workspace smaller
 *   than lnh_marching_cubes_workspace_size(nx, ny, nz) (4-byte aligned, contents irrelevant; 0 for a refused size), a
 *   capacity of 0; LNH_ERR_UNSUPPORTED for nx * ny * nz >= 2^31 and max_vertices >= 2^31.
 */
LNH_API uint64_t lnh_marching_cubes_workspace_size(uint32_t nx, uint32_t ny, uint32_t nz);
LNH_API int lnh_marching_cubes_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *ws,
                                     uint64_t ws_bytes, uint32_t *counts, lnh_stream_t stream);
LNH_API int lnh_marching_cubes_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float iso, void *ws,
                                    uint64_t ws_bytes, float *vertices, uint32_t max_vertices, int32_t *triangles,
                                    uint32_t max_triangles, lnh_stream_t stream);

/* ---- mesh baseline fit: projective TSDF fusion of range images, and the trim of the mesh to what was observed — csrc/tsdf.hip.
 * (Added without moving lnh_version: detect by symbol.)  The meshing function of LidarNVSMeshing.fit
 * (lidarnvs/lidarnvs_meshing.py) for a sequence of range images with poses; nearest-pixel depth, unit weights, the column
 * wrap, the fill and the trim are this package's own, not Open3D's.
 * Lattice: point (ix, iy, iz) at lo[a] + float(i_a) * step[a]; every lattice array is [nx, ny, nz], z fastest, as
 *   lnh_marching_cubes_* reads it.  lo and step are HOST arrays of 3 floats.
 * lnh_tsdf_integrate: panos f32 [F,H,W] (a depth <= 0 or not finite: no observation), world_to_lidar f32 [F,12] (the affine
 *   3 x 4 matrix of each frame, row-major), lidar_K = (fov_up, fov) in degrees.  sum f32 [n] and count u32 [n] are read, added
 *   to and written back.  For every lattice point, the frames in order 0 .. F-1, all in fp32 with one rounded operation per
 *   operator and nothing contracted:
 *     p_a = lo[a] + float(i_a) * step[a]
 *     q_r = ((m[r][0] * p_x + m[r][1] * p_y) + m[r][2] * p_z) + m[r][3]                       r = x, y, z
 *     r   = sqrt((q_x q_x + q_y q_y) + q_z q_z); the frame is skipped unless 0 < r < max_depth
 *     the pixel is lnh_lidar_to_pano's (csrc/pano_geom.h): beta = f32(pi) - f32(atan2(q_y, q_x)), alpha = f32(atan2(q_z,
 *       sqrt(q_x q_x + q_y q_y))) + down_rad, column = rint(beta / col_step), row = rint(float(H) - alpha / row_step), atan2 in
 *       double; skipped outside the rows [0, H).  The one difference: a column that rounds to W is column 0
 *     d   = panos[f][row][column]; skipped unless 0 < d < inf
 *     s   = d - r; skipped if s < -trunc
 *     sum += min(s / trunc, 1); count += 1
 *   One thread owns a lattice point: no atomics, the result is a function of the inputs alone, and the frames split over several
 *   calls give the bits of one call.  A wave covers a 4 x 4 x 4 brick of lattice points.
 * lnh_tsdf_finalize: volume f32 [n] = -(sum / float(count)) where count >= min_count (>= 1), else the fill +1.  Free space is
 *   negative — the BELOW side of lnh_marching_cubes_* at iso 0, so the normals face the sensors — and all unobserved points are
 *   equal, so no cell made only of them crosses.  (float(count) is exact below 2^24 frames.)
 * lnh_mesh_vertex_observed: vertices f32 [V,3] in index units -> keep u8 [V] = 1 iff every lattice point of the smallest lattice
 *   edge / face / cell holding the vertex has count >= min_count: for a marching-cubes vertex the two ends of its edge, for a
 *   vertex exactly on a lattice point that one point.  0 for a vertex outside [0, n_a - 1] or NaN (compared in integers behind
 *   the floor, so a dimension above 2^24 is safe).
 * lnh_mesh_filter_count / _emit: Open3D's remove_vertices_by_mask with keep = 1 meaning "stays".  The kept vertices in order; the
 *   triangles whose three indices are in [0, V) and kept, in order, renumbered.  Integers only.  count writes counts u32[4]
 *   (device) = kept vertices, kept triangles, 0, 0 and leaves in the workspace what emit reads: call emit after it on the same
 *   stream with the same keep, triangles and workspace.  emit never writes past max_vertices / max_triangles rows; a mask of all
 *   zeros gives counts 0, 0 and needs no emit (max_vertices = 0 is refused; max_triangles = 0 writes the vertices alone).
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null pointer, F, H, W or V or T = 0, a lattice dimension below 2, a trunc
 *   or step that is not positive and finite, a lo that is not finite, fov <= 0, min_count = 0, a workspace smaller than
 *   lnh_mesh_filter_workspace_size(V, T) (4-byte aligned, contents irrelevant; 0 for a refused size);
 *   LNH_ERR_UNSUPPORTED for nx * ny * nz >= 2^31, H * W > 2^24, V or T >= 2^31.
 */
LNH_API int lnh_tsdf_integrate(const float *panos, const float *world_to_lidar, uint32_t F, uint32_t H, uint32_t W, float fov_up,
                               float fov, float max_depth, const float *lo, const float *step, uint32_t nx, uint32_t ny,
                               uint32_t nz, float trunc, float *sum, uint32_t *count, lnh_stream_t stream);
LNH_API int lnh_tsdf_finalize(const float *sum, const uint32_t *count, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t min_count,
                              float *volume, lnh_stream_t stream);
LNH_API int lnh_mesh_vertex_observed(const float *vertices, uint32_t V, const uint32_t *count, uint32_t nx, uint32_t ny,
                                     uint32_t nz, uint32_t min_count, uint8_t *keep, lnh_stream_t stream);
LNH_API uint64_t lnh_mesh_filter_workspace_size(uint32_t V, uint32_t T);
LNH_API int lnh_mesh_filter_count(const uint8_t *keep, uint32_t V, const int32_t *triangles, uint32_t T, void *ws,
                                  uint64_t ws_bytes, uint32_t *counts, lnh_stream_t stream);
LNH_API int lnh_mesh_filter_emit(const float *vertices, const uint8_t *keep, uint32_t V, const int32_t *triangles, uint32_t T,
                                 void *ws, uint64_t ws_bytes, float *out_vertices, uint32_t max_vertices, int32_t *out_triangles,
                                 uint32_t max_triangles, lnh_stream_t stream);

/* ---- mesh ray casting: watertight closest hit.  (Added without moving lnh_version: detect by symbol.)
 * Replaces RaycastingScene.cast_rays (Open3D / Embree on the host) of lidarnvs/lidarnvs_meshing.py:293-353.
 * Mesh: vertices f32 [V,3], triangles i32 [T,3].  Rays: rays_o, rays_d f32 [N,3]; d need not be normalised.
 * The intersection function (fp32, one rounded operation per operator, nothing contracted), after Woop, Benthin, Wald,
 * "Watertight Ray/Triangle Intersection", JCGT 2013:
 *   kz = axis of the largest |d| (ties: the lowest axis); kx = (kz + 1) % 3, ky = (kx + 1) % 3, swapped when d[kz] < 0
 *   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
 *   per vertex P of (A, B, C) = (v0, v1, v2): Pkx = P[kx] - o[kx], Pky = P[ky] - o[ky], Pkz = P[kz] - o[kz],
 *     Px = Pkx - Sx * Pkz, Py = Pky - Sy * Pkz
 *   U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax; if one of them == 0, all three again from the same
 *     fp32 operands in double (exact products, the difference rounded to double), each converted to fp32
 *   miss if their signs are mixed (two-sided, no culling); det = (U + V) + W, miss if det == 0
 *   Pz = Sz * Pkz, t = ((U * Az + V * Bz) + W * Cz) / det; miss unless t >= 0 and finite; -0 is stored as +0
 *   t is in units of |d| as given (Open3D's t_hit).  A ray with a zero or non-finite direction or a non-finite origin misses.
 * Answer for a ray: the minimum over all triangles that hit of the key (bits of t) << 32 | triangle index — the nearest
 *   hit, among equal t (a shared edge or vertex) the smallest index.  This tie rule and the orientation of the normal are this
 *   library's own; Embree's are not pinned.
 *   t_hit f32 [N] (+inf on a miss), primitive_ids i32 [N] (-1), primitive_normals f32 [N,3]: with e1 = v1 - v0, e2 = v2 - v0,
 *   n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), len = sqrtf((nx nx + ny ny) + nz nz), n / len (zeros on a
 *   miss and when len is 0 or not finite); incidences f32 [N] = |(d0 n0 + d1 n1) + d2 n2| (0 on a miss; NULL: not written).
 * Acceleration: a uniform grid of nx x ny x nz cells (1 ... 1024 each) over the vertices' bounding box.  For every ray and
 *   every grid the result is exactly the minimum key over ALL triangles; nx = ny = nz = 1 reads the triangle
 *   array itself.  The order of the entries inside a cell is arrival order and no output depends on it.
 * lnh_raycast_bounds: box f32[9] (device) = min[3], max[3] of the finite vertex coordinates (exact, no atomics) and the largest
 *   extent of one triangle per axis; counts u32[4] = non-finite vertex coordinates, triangle indices outside [0, V), 0, 0.
 *   A scene with a non-zero count must not be built further.
 * lnh_raycast_build_count: cell_start u32[nx*ny*nz + 1] (exclusive scan of the per-cell list lengths; integer atomics only),
 *   counts[2], counts[3] = low and high word of the 64-bit entry total.  The caller reads it, refuses a total above
 *   2^31 - 1, allocates cell_tris u32[entries] and calls lnh_raycast_build_fill with the same mesh, box, grid and cell_start.
 * lnh_raycast_cast: one thread per ray, no host read, no allocation (capturable).  Never writes outside the N rows.
 * workspace: lnh_raycast_workspace_size(V, T, nx, ny, nz, entries) bytes, 4-byte aligned, contents irrelevant; serves the
 *   three build calls (0 for a refused size).
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null pointer, an empty mesh (V or T = 0), a grid dimension of 0,
 *   entries = 0, a workspace too small; LNH_ERR_UNSUPPORTED for V, T or N >= 2^31, more than 1024 cells on an axis, entries
 *   above 2^31 - 1.
 */
LNH_API uint64_t lnh_raycast_workspace_size(uint32_t V, uint32_t T, uint32_t nx, uint32_t ny, uint32_t nz, uint64_t entries);
LNH_API int lnh_raycast_bounds(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, void *ws,
                               uint64_t ws_bytes, float *box, uint32_t *counts, lnh_stream_t stream);
LNH_API int lnh_raycast_build_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *box,
                                    uint32_t nx, uint32_t ny, uint32_t nz, void *ws, uint64_t ws_bytes, uint32_t *cell_start,
                                    uint32_t *counts, lnh_stream_t stream);
LNH_API int lnh_raycast_build_fill(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *box,
                                   uint32_t nx, uint32_t ny, uint32_t nz, void *ws, uint64_t ws_bytes,
                                   const uint32_t *cell_start, uint32_t *cell_tris, uint64_t entries, lnh_stream_t stream);
LNH_API int lnh_raycast_cast(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t T, const float *box,
                             uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *cell_start, const uint32_t *cell_tris,
                             uint64_t entries, const float *rays_o, const float *rays_d, uint32_t N, float *t_hit,
                             int32_t *primitive_ids, float *primitive_normals, float *incidences, lnh_stream_t stream);

/* ---- exact k-nearest neighbours of a point cloud over a uniform grid.  (Added without moving lnh_version: detect by symbol.)
 * Replaces KDTreeFlann.search_knn_vector_3d (Open3D on the host, one call per hit point) and the np.mean over the neighbours'
 * intensities of lidarnvs/lidarnvs_meshing.py:132-140 (predict_frame).
 * Cloud: points f32 [N,3].  Queries: queries f32 [Q,3], 1 <= k <= 16.
 * The distance (fp32, one rounded operation per operator, nothing contracted):
 *   dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z, d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
 * Answer for a query: the min(k, N) smallest keys (bits of d2) << 32 | point index over ALL points, in ascending key order —
 *   nearest first, among equal distances the smallest index (d2 >= 0: its bit pattern orders like its value).  This tie rule
 *   is this library's own; KDTreeFlann's is not pinned.
 *   indices i32 [Q,k], dist2 f32 [Q,k] (squared distances); either may be NULL; ranks >= min(k, N) hold -1 / +inf.
 *   values f32 [N] and mean f32 [Q] go together (both or NULL): mean = the sum of the neighbours' values in rank order,
 *   accumulated in fp64, divided by their count, rounded once to fp32.
 *   valid u8 [Q] (NULL: every query): a query with valid == 0, or with a non-finite coordinate, gets -1 / +inf / mean 0.
 * Acceleration: a uniform grid of nx x ny x nz cells (1 ... 1024 each) over the points' bounding box.  For every query and every
 *   grid the outputs are bit-identical to those of nx = ny = nz = 1, which reads the point array itself (DESIGN §16 has the
 *   stopping rule and its argument: no ulp slack anywhere).  The order of the points inside a cell is arrival order and no output
 *   depends on it.
 * lnh_knn_bounds: box, 8 words on the device = min[3], max[3] of the finite coordinates as f32 (exact, no atomics), then the
 *   count of non-finite coordinates as u32 (saturating), then 0.  A cloud with a non-zero count must not be built further.
 *   The caller reads the box (the one host read of a build) to choose a grid.
 * lnh_knn_build_count: cell_start u32[nx*ny*nz + 1] (exclusive scan of the per-cell counts; integer atomics only) and
 *   slabs f32[2 * (nx + ny + nz)]: per axis (x, then y, then z) smin[i] = the smallest coordinate of the points whose cell index
 *   along the axis is >= i (+inf where there is none), then in the same layout pmax[i] = the largest coordinate of the points
 *   whose cell index is <= i (-inf).
 * lnh_knn_build_fill: sorted f32 [N,4] (16-byte aligned), the points ordered by cell as rows (x, y, z, bits of the original
 *   index); same cloud, box, grid and cell_start as the count.
 * lnh_knn_search: one thread per query, ONE launch, no host read, no allocation (capturable).  Never writes outside the Q rows.
 * workspace: lnh_knn_workspace_size(N, nx, ny, nz) bytes, 4-byte aligned, contents irrelevant; serves the three build calls (0 for
 *   a refused size).
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null pointer, an empty cloud (N = 0), a grid dimension of 0, k outside
 *   1 ... 16, values without mean or mean without values, no output at all, a workspace too small; LNH_ERR_UNSUPPORTED for N or
 *   Q >= 2^31, more than 1024 cells on an axis.
 */
LNH_API uint64_t lnh_knn_workspace_size(uint32_t N, uint32_t nx, uint32_t ny, uint32_t nz);
LNH_API int lnh_knn_bounds(const float *points, uint32_t N, void *ws, uint64_t ws_bytes, float *box, lnh_stream_t stream);
LNH_API int lnh_knn_build_count(const float *points, uint32_t N, const float *box, uint32_t nx, uint32_t ny, uint32_t nz,
                                void *ws, uint64_t ws_bytes, uint32_t *cell_start, float *slabs, lnh_stream_t stream);
LNH_API int lnh_knn_build_fill(const float *points, uint32_t N, const float *box, uint32_t nx, uint32_t ny, uint32_t nz,
                               void *ws, uint64_t ws_bytes, const uint32_t *cell_start, float *sorted, lnh_stream_t stream);
LNH_API int lnh_knn_search(const float *points, uint32_t N, const float *box, uint32_t nx, uint32_t ny, uint32_t nz,
                           const uint32_t *cell_start, const float *sorted, const float *slabs, const float *queries,
                           const uint8_t *valid, uint32_t Q, uint32_t k, const float *values, int32_t *indices, float *dist2,
                           float *mean, lnh_stream_t stream);

/* ---- the ray-drop MLP of the PCGen baseline (lidarnvs/raydrop_train_pcgen.py: RayDrop, run_network with the
 * identity embedding, img2mse / l1loss, torch.optim.Adam) — csrc/raydrop.hip.  Everything is fp32; no operand is narrowed.
 * params: ONE flat buffer in torch's nn.Linear layout, 16-byte aligned: for hidden layer l = 0 .. D-1 weight[l] [W, in_l]
 *   row-major (in_0 = 5, else W) then bias[l] [W]; then output.weight [1, W] and output.bias [1].
 *   lnh_raydrop_param_count(D, W) = 5 W + W + (D - 1)(W^2 + W) + W + 1 floats (0 for an unsupported shape).
 *   Supported: W 128 or 256, 1 <= D <= 8; anything else returns LNH_ERR_INVALID_ARG.
 * rows: [N, stride] f32, stride >= 5: direction x, y, z, depth, intensity, [target] (lnh_raydrop_grad: stride 6).  A row at or
 *   behind N is never read.
 * lnh_raydrop_forward: out[N] = the raw network output (no sigmoid).  One launch.
 * lnh_raydrop_grad: forward, loss, backward and every weight and bias gradient of rows [B, 6]; two launches.
 *   loss_type 0: e_i = (out_i - t_i)^2 (img2mse, mseloss), 1: |out_i - t_i| (l1loss).  loss[0] = (sum_i e_i) / B with one
 *   division.  The backward carries the unnormalised output gradient 2 (out_i - t_i) (L1: sign, 0 at 0); every element of
 *   grad[P] is its sum over the batch divided by B once, and is OVERWRITTEN.  No float atomics: loss and grad are functions of
 *   (params, rows, B) alone — the order of every sum depends on B, D and W only — and two calls are bit-identical.
 *   ws: lnh_raydrop_workspace_size(D, W, B) bytes (0 for a refused shape or B), 16-byte aligned, contents irrelevant.
 * lnh_raydrop_adam: torch.optim.Adam (no weight decay, no amsgrad) on the flat buffer.  The step count lives on the device,
 *   double-buffered (step_in != step_out, one float each, as in lnh_adam_table_step): t = *step_in is the count BEFORE this
 *   step, *step_out = t + 1, and the learning rate is lr_table[min(t, lr_len - 1)], read from device memory.
 * No call reads the host or allocates; all three can be captured in a hipGraph. */
LNH_API uint64_t lnh_raydrop_param_count(uint32_t D, uint32_t W);
LNH_API uint64_t lnh_raydrop_workspace_size(uint32_t D, uint32_t W, uint32_t B);
LNH_API int lnh_raydrop_forward(const float *params, uint32_t D, uint32_t W, const float *rows, uint32_t stride, uint32_t N,
                                float *out, lnh_stream_t stream);
LNH_API int lnh_raydrop_grad(const float *params, uint32_t D, uint32_t W, const float *rows, uint32_t B, uint32_t loss_type,
                             void *ws, uint64_t ws_bytes, float *loss, float *grad, lnh_stream_t stream);
LNH_API int lnh_raydrop_adam(float *params, float *exp_avg, float *exp_avg_sq, const float *grad, uint32_t P,
                             const float *lr_table, uint32_t lr_len, const float *step_in, float *step_out, double beta1,
                             double beta2, double eps, lnh_stream_t stream);

/* ---- the ray-drop U-Net of the mesh baselines (README f11; lidarnvs/unet.py: UNet(10, 1, bilinear=False) in eval mode,
 * the reference's --amp arithmetic) — csrc/unet.hip.  Inference only.
 * Activations: fp16, NHWC [N, H, W, C] with C a multiple of 32.  Weights: fp16, rounded to nearest even from fp32.  Every
 *   product sum of the convolutions is accumulated in fp32 on v_mfma_f32_16x16x32_f16, k in the order (tap row-major, source 0
 *   channels, source 1 channels); no float atomics, no partial sums in memory: an output is a function of (packed parameters,
 *   input, tile) alone and two calls are bit-identical.  No call reads the host or allocates; all can be captured in a hipGraph.
 *   Every pointer must be 16-byte aligned.  N H W of any image at most 2^26.
 * lnh_unet_workspace_size(N, H, W): bytes of every activation buffer of one forward of the whole net on [N, 10, H, W] (the
 *   layout is lidarnerf/unet.py: workspace_layout; every buffer 256-byte aligned); 0 for a refused shape (N = 0, H or W < 16,
 *   N H W > 2^26).
 * lnh_unet_input: in [N, C, H, W] f32 (1 <= C <= 32) -> out [N, H, W, 32] fp16, channels C .. 31 zero.
 * lnh_unet_conv3x3: 3 x 3 convolution, padding 1, no bias, of the channel concatenation (src0, src1), then eval-mode BatchNorm
 *   and ReLU in fp32: out[n, y, x, co] = fp16(max(fmaf(acc, scale[co], shift[co]), 0)), out [N, H, W, Cout].
 *   src0 [N, H0, W0, C0]: pool = 0: H0 = H, W0 = W.  pool = 1: the 2 x 2 maximum of src0 is taken on read (MaxPool2d(2));
 *     H = H0 / 2, W = W0 / 2 (floor: an odd last row or column is dropped).
 *   src1 [N, H1, W1, C1] or NULL (C1 = 0): channels C0 .. C0 + C1 - 1 (torch.cat([skip, upsampled])), placed top-left, reading as
 *     zero for y >= H1 or x >= W1 (F.pad); H - H1 and W - W1 must be 0 or 1.
 *   weight [Cout, 9, C0 + C1] fp16 (torch's [Cout, Cin, 3, 3] with the channel last); scale, shift [Cout] f32.
 *   C0, C1 multiples of 32 up to 1024 (C0 >= 32), Cout a multiple of 64 up to 1024.
 *   tile: 0 = chosen from the shape; LNH_UNET_TILE_16 / _32 / _64: pixels per wave, four waves of a workgroup on neighbouring
 *     pixel tiles and the same 64 output channels; LNH_UNET_TILE_KSPLIT: 16 pixels per workgroup, its four waves share the k
 *     range and add their partial sums through LDS in the fixed order (w0 + w1) + (w2 + w3).  The first three give the same
 *     bits; the last may differ from them in the last place of the fp32 sum.
 * lnh_unet_upconv2x2: ConvTranspose2d(kernel 2, stride 2) with bias: in [N, H, W, Cin] -> out [N, 2H, 2W, Cout],
 *   out[n, 2y+dy, 2x+dx, co] = fp16(bias[co] + sum_ci in[n, y, x, ci] weight[2dy + dx, co, ci]); weight [4, Cout, Cin] fp16 (torch's
 *   [Cin, Cout, 2, 2] permuted), bias [Cout] f32.  Cin a multiple of 32 up to 1024, Cout a multiple of 64 up to 1024.
 * lnh_unet_head: the 1 x 1 output convolution: in [N, H, W, 64] fp16, weight [64] fp16, bias [1] f32 (read on the device) ->
 *   logits [N, 1, H, W] f32 = bias + the fmaf chain over channel 0 .. 63 in fp32; mask (or NULL) [N, 1, H, W] f32 = 1 where
 *   logit > 0 (sigmoid(logit) > 0.5), else 0 — also for a NaN logit. */
#define LNH_UNET_TILE_16 1u
#define LNH_UNET_TILE_32 2u
#define LNH_UNET_TILE_64 4u
#define LNH_UNET_TILE_KSPLIT 8u
LNH_API uint64_t lnh_unet_workspace_size(uint32_t N, uint32_t H, uint32_t W);
LNH_API int lnh_unet_input(const float *in, uint32_t N, uint32_t C, uint32_t H, uint32_t W, void *out, lnh_stream_t stream);
LNH_API int lnh_unet_conv3x3(const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool, const void *src1,
                             uint32_t C1, uint32_t H1, uint32_t W1, const void *weight, const float *scale,
                             const float *shift, uint32_t N, uint32_t Cout, uint32_t tile, void *out, lnh_stream_t stream);
LNH_API int lnh_unet_upconv2x2(const void *in, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, const void *weight,
                               const float *bias, uint32_t Cout, void *out, lnh_stream_t stream);
LNH_API int lnh_unet_head(const void *in, uint32_t N, uint32_t H, uint32_t W, const void *weight, const float *bias,
                          float *logits, float *mask, lnh_stream_t stream);

/* ---- U-Net training (README f12) — csrc/unet_train.hip, csrc/unet_train_conv.hip, csrc/unet_train_wgrad.hip (and
 * the RAW epilogue of csrc/unet.hip).
 * The max-pool and head backward, the transposed convolution's weight pack, data gradient and weight / bias gradient, and the
 * training-mode convolution layer: weight pack, raw convolution (forward and data gradient), batch statistics, BatchNorm + ReLU
 * and their backward, the weight gradient.
 * Activations and activation gradients: fp16 NHWC, rounded once per tensor; parameter gradients f32.  No float atomics: a sum that
 * is split goes to a workspace as partials and is added in a fixed order, so two calls give the same bits.  No call reads the host
 * or allocates.  N H W of any image at most 2^26.
 * lnh_unet_pool_backward: the gradient of MaxPool2d(2) at x [N, H0, W0, C] fp16 for dpool [N, H0 / 2, W0 / 2, C] fp16 (floor):
 *   dx[n, y, x, c] = fp16(route + skip) in fp32, where route = dpool of the element's window if the element is the FIRST maximum of
 *   that 2 x 2 window in row-major order (strict >, and a NaN takes over from any earlier value: torch's rule), else 0 — also 0 in a last odd row or column, which no window
 *   covers — and skip = dskip[(n, y, x) skip_stride + c], or 0 with dskip NULL (then skip_stride = 0).  dskip is read in place from
 *   a tensor with skip_stride >= C channels per pixel (a multiple of 8, up to 2048): channels [0, C) of the data gradient of the
 *   concatenating convolution.  C a multiple of 32, 32 .. 1024; H0, W0 >= 2.  One owner per element.
 * lnh_unet_head_backward: the 1 x 1 head.  a [N, H, W, 64] fp16 (the head's input), weight [64] fp16 (as lnh_unet_head reads it),
 *   dlogits [N, 1, H, W] f32, used as given (loss scaling is the caller's; non-finite values pass through) ->
 *   dx [N, H, W, 64] fp16 = fp16(dlogit[p] weight[c]) (one fp32 product);
 *   dweight [64] f32 = sum_p fp32(dlogit[p] a[p, c]); dbias [1] f32 = sum_p dlogit[p].  The sums: the 64 consecutive pixels
 *   64 k .. 64 k + 63 are added in fp32 by the xor butterfly (lane i with lane i ^ 32, then ^ 16, .. ^ 1), those partials go to
 *   ws and are added in ascending k in float64, the result rounded to f32.
 *   ws: lnh_unet_head_backward_workspace_size(N, H, W) = ceil(N H W / 64) x 65 x 4 bytes (0: refused shape), 16-byte aligned.
 * lnh_unet_pack_upconv: weight f32 [Cin, Cout, 2, 2] (the ConvTranspose2d parameter itself) -> fwd fp16 [4, Cout, Cin], the image
 *   lnh_unet_upconv2x2 reads (fwd[2dy + dx, co, ci] = fp16(weight[ci, co, dy, dx])), and, unless bwd is NULL, bwd fp16
 *   [Cin, 4, Cout] with bwd[ci, 2dy + dx, co] the same value: the image of the data gradient.  Cin, Cout multiples of 64 up to 1024.
 * lnh_unet_upconv2x2_backward_data: dx [N, H, W, Cin] fp16 = fp16(sum_{q, co} dy[n, 2y + (q >> 1), 2x + (q & 1), co] bwd[ci, q, co]),
 *   fp32 sums on the MFMA, k in the order (q, co).  dy is read in place: channels [dy_offset, dy_offset + Cout) of an fp16 tensor
 *   [N, Hd, Wd, dy_stride] with Hd - 2H and Wd - 2W each 0 or 1 (the gradient at a padded last row / column is dropped); offset and
 *   stride multiples of 8, stride up to 2048.  Cin a multiple of 64, Cout a multiple of 32, both up to 1024.
 * lnh_unet_upconv2x2_backward_weight: dweight f32 [Cin, Cout, 2, 2] (the parameter's layout; overwritten) with dweight[ci, co, q] =
 *   sum over the M = N H W input pixels p of x[p, ci] dy[2p + q, co], fp32 sums on the MFMA, and dbias f32 [Cout] = the sum of dy
 *   over the 4 M output pixels.  x [N, H, W, Cin] fp16; dy read in place as in lnh_unet_upconv2x2_backward_data.  Cin, Cout
 *   multiples of 64 up to 1024.  The pixel range is cut into S = min(ceil(M / 256), max(1, floor(16 MiB / (16 Cin Cout)))) slices
 *   of L = ceil(M / S) rounded up to 32 pixels (then S = ceil(M / L)); within a slice the sums run over steps of 32 pixels in
 *   ascending order (dbias: per step q, then pixel, ascending, one fp32 chain); the slices go to ws and are added in ascending order
 *   in float64.  ws: lnh_unet_upconv2x2_backward_weight_workspace_size(N, H, W, Cin, Cout) = S (4 Cin Cout + Cout) x 4 bytes
 *   (0: refused shape), 16-byte aligned.  Same shape, same bits. */
LNH_API int lnh_unet_pool_backward(const void *x, uint32_t N, uint32_t H0, uint32_t W0, uint32_t C, const void *dpool,
                                   const void *dskip, uint32_t skip_stride, void *dx, lnh_stream_t stream);
LNH_API int lnh_unet_pack_upconv(const float *weight, uint32_t Cin, uint32_t Cout, void *fwd, void *bwd, lnh_stream_t stream);
LNH_API int lnh_unet_upconv2x2_backward_data(const void *dy, uint32_t Hd, uint32_t Wd, uint32_t dy_stride, uint32_t dy_offset,
                                             uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout, const void *weight,
                                             void *dx, lnh_stream_t stream);
LNH_API uint64_t lnh_unet_upconv2x2_backward_weight_workspace_size(uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout);
LNH_API int lnh_unet_upconv2x2_backward_weight(const void *x, const void *dy, uint32_t Hd, uint32_t Wd, uint32_t dy_stride,
                                               uint32_t dy_offset, uint32_t N, uint32_t H, uint32_t W, uint32_t Cin, uint32_t Cout,
                                               void *ws, uint64_t ws_bytes, float *dweight, float *dbias, lnh_stream_t stream);
LNH_API uint64_t lnh_unet_head_backward_workspace_size(uint32_t N, uint32_t H, uint32_t W);
LNH_API int lnh_unet_head_backward(const void *a, uint32_t N, uint32_t H, uint32_t W, const void *weight, const float *dlogits,
                                   void *ws, uint64_t ws_bytes, void *dx, float *dweight, float *dbias, lnh_stream_t stream);
/* The training-mode convolution layer, a = relu(bn(z)), z = fp16(conv3x3(x)), BatchNorm on the statistics of the batch.
 * lnh_unet_pack_conv3x3: weight f32 [Cout, Cin, 3, 3] (the Conv2d parameter itself) -> fwd fp16 [Cout, 9, Cpad], the image
 *   lnh_unet_conv3x3 reads (fwd[co, t, ci] = fp16(weight[co, ci, t]), channels Cin .. Cpad - 1 zero; Cpad = 32 for Cin <= 32, else
 *   Cin, which must then be a multiple of 32 up to 1024), and, unless bwd is NULL, bwd fp16 [Cin, 9, Cout] with bwd[ci, t, co] =
 *   fp16(weight[co, ci, 8 - t]): the flipped and transposed image, on which the same convolution is the data gradient.  bwd needs
 *   Cin % 64 == 0.  Cout a multiple of 64 up to 1024.
 * lnh_unet_conv3x3_raw: lnh_unet_conv3x3 without scale / shift: out = fp16(acc), the same main loop, sources, pool on read, padding
 *   rule, tile argument and tile rule.  As the data gradient: dx = conv3x3_raw(dz, bwd) with C0 = the layer's Cout, no pool, no second
 *   source and Cout = the layer's C0 + C1; for a pooling layer dx is the gradient of the pooled tensor (lnh_unet_pool_backward's
 *   dpool), for a concatenating layer [N, H, W, C0 + C1], which lnh_unet_pool_backward (skip channels) and
 *   lnh_unet_upconv2x2_backward_* (offset C0) read in place.
 * lnh_unet_bn_stats: z fp16 [M, C] (M = N H W >= 2, C a multiple of 32 up to 1024), gamma, beta f32 [C] -> mean, invstd f32 [C]
 *   (saved for the backward), scale = gamma invstd, shift = beta - mean scale f32 [C], and in place unless NULL running_mean <-
 *   (1 - momentum) running_mean + momentum mean, running_var <- (1 - momentum) running_var + momentum var M / (M - 1).  The
 *   statistics are those of the rounded z.  sum z and sum z^2 in float64 (an fp16 square is exact there), in a fixed order: with
 *   P = 256 ceil(M / 2^14) pixels per partial (at most 64 partials), row r = 0 .. 31 of partial k chains the pixels k P + r,
 *   k P + r + 32, ..; the rows of a partial are added in ascending r, the partials go to ws and are added in ascending k.  mean = S1 / M, var =
 *   max(S2 / M - mean^2, 0) (biased; a NaN stays), invstd = 1 / sqrt(var + eps), scale, shift (from the unrounded scale) and the
 *   running statistics are formed in float64 and rounded once to f32.  ws: lnh_unet_bn_stats_workspace_size(M, C) =
 *   ceil(M / P) x 2 C x 8 bytes (0: refused shape), 16-byte aligned.
 * lnh_unet_bn_relu: a [M, C] fp16 = fp16(max(fmaf(float(z), scale[c], shift[c]), 0)): the epilogue of lnh_unet_conv3x3 on the stored z.
 * lnh_unet_bn_relu_backward: with g = da [a > 0] and xhat = (float(z) - mean) invstd in fp32: dbeta f32 [C] = sum g, dgamma f32 [C] =
 *   sum fp32(g xhat), both added in float64 in the order of lnh_unet_bn_stats and rounded once; then dz [M, C] fp16 =
 *   fp16(scale ((g - dbeta / M) - xhat (dgamma / M))) in fp32 from those rounded sums.  dz may be da (one owner per element, read
 *   before written).  Linear in da: loss scaling is the caller's; non-finite values pass through.  ws:
 *   lnh_unet_bn_relu_backward_workspace_size(M, C), the same figure. */
LNH_API int lnh_unet_pack_conv3x3(const float *weight, uint32_t Cout, uint32_t Cin, void *fwd, void *bwd, lnh_stream_t stream);
LNH_API int lnh_unet_conv3x3_raw(const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool, const void *src1,
                                 uint32_t C1, uint32_t H1, uint32_t W1, const void *weight, uint32_t N, uint32_t Cout,
                                 uint32_t tile, void *out, lnh_stream_t stream);
LNH_API uint64_t lnh_unet_bn_stats_workspace_size(uint64_t M, uint32_t C);
LNH_API int lnh_unet_bn_stats(const void *z, uint64_t M, uint32_t C, const float *gamma, const float *beta, double eps,
                              double momentum, void *ws, uint64_t ws_bytes, float *mean, float *invstd, float *scale,
                              float *shift, float *running_mean, float *running_var, lnh_stream_t stream);
LNH_API int lnh_unet_bn_relu(const void *z, uint64_t M, uint32_t C, const float *scale, const float *shift, void *a,
                             lnh_stream_t stream);
LNH_API uint64_t lnh_unet_bn_relu_backward_workspace_size(uint64_t M, uint32_t C);
LNH_API int lnh_unet_bn_relu_backward(const void *z, const void *a, const void *da, uint64_t M, uint32_t C, const float *mean,
                                      const float *invstd, const float *scale, void *ws, uint64_t ws_bytes, void *dz,
                                      float *dgamma, float *dbeta, lnh_stream_t stream);
/* The 3 x 3 convolution's weight gradient — csrc/unet_train_wgrad.hip.
 * lnh_unet_conv3x3_backward_weight: dweight f32 [Cout, Cin, 3, 3] (the parameter's layout; overwritten) with dweight[co, ci, t] =
 *   sum over the M = N H W output pixels p of dz[p, co] X[p + off(t), ci], t the forward tap (fwd[co, t, ci]).  X is the operand
 *   lnh_unet_conv3x3 read, formed on read and never stored: src0 [N, H0, W0, C0] fp16, max-pooled 2 x 2 with pool = 1 (floor), then
 *   the channels of src1 [N, H1, W1, C1] fp16 (zero for y >= H1 or x >= W1; H - H1, W - W1 each 0 or 1); a tap outside the image is
 *   zero.  dz [N, H, W, Cout] fp16.  C1 = 0 or C1 = C0; C0 = 32 (the padded first layer, C1 = 0, Cin = 1 .. 32 real channels: channels
 *   Cin .. 31 are not written) or a multiple of 64 up to 1024 (Cin = C0 + C1); Cout a multiple of 64 up to 1024; every pointer
 *   16-byte aligned.  fp32 sums on the MFMA, no float atomics.  The pixel range is cut into
 *   S = min(ceil(M / 256), max(1, floor(32 MiB / (36 (C0 + C1) Cout)))) slices of L = ceil(M / S) rounded up to 32 pixels (then
 *   S = ceil(M / L)); within a slice the sums run over steps of 32 pixels in ascending order; the slices go to ws as
 *   [S][9][Cout][C0 + C1] f32 and are added in ascending order in float64, rounded once.  variant: how the MFMA operands leave the
 *   LDS — 0 = the default (LNH_UNET_WGRAD_TR), LNH_UNET_WGRAD_GATHER = 16-bit reads, LNH_UNET_WGRAD_TR = ds_read_b64_tr_b16; the
 *   two give the same bits.  ws: lnh_unet_conv3x3_backward_weight_workspace_size(N, H0, W0, pool, C0, C1, Cout) = S x 36 (C0 + C1)
 *   Cout bytes (0: refused shape).  Same shape, same bits; a non-finite dz makes the 9 Cin entries of its co non-finite, no others. */
#define LNH_UNET_WGRAD_GATHER 1u
#define LNH_UNET_WGRAD_TR 2u
LNH_API uint64_t lnh_unet_conv3x3_backward_weight_workspace_size(uint32_t N, uint32_t H0, uint32_t W0, uint32_t pool, uint32_t C0,
                                                                 uint32_t C1, uint32_t Cout);
LNH_API int lnh_unet_conv3x3_backward_weight(const void *src0, uint32_t C0, uint32_t H0, uint32_t W0, uint32_t pool,
                                             const void *src1, uint32_t C1, uint32_t H1, uint32_t W1, const void *dz, uint32_t N,
                                             uint32_t Cout, uint32_t Cin, uint32_t variant, void *ws, uint64_t ws_bytes,
                                             float *dweight, lnh_stream_t stream);
/* The training step around forward and backward — csrc/unet_train_step.hip.  No float atomics, no host read, no allocation; every
 * sum is taken in an order that depends on the sizes alone, so two calls give the same bits; capturable.
 * lnh_unet_loss_grad: the loss of raydrop_train_poisson.py for the one-class net and its cotangent in closed form.  logits f32 [M]
 *   (M = N H W, 1 .. 2^26), masks [M] holding 0 / 1 as f32 (LNH_UNET_MASK_F32) or uint8 (LNH_UNET_MASK_U8) ->
 *   loss[0] f32 = mean BCE-with-logits + 1 - dice(sigmoid(x), t) over the whole batch (reduce_batch_first, epsilon e = 1e-6) and
 *   dlogits f32 [M] = loss_scale dL/dx.  With s = sigmoid(x), I = sum s t, S = sum (s + t):
 *   dL/dx_i = (s_i - t_i) / M - s_i (1 - s_i) (2 t_i (S + e) - (2 I + e)) / (S + e)^2, the dice part exactly 0 when S == 0 (then
 *   dice = 1: dice_coeff's masked_fill).  BCE_i = max(x, 0) - x t + log1p(exp(-|x|)); s (1 - s) = exp(-|x|) / (1 + exp(-|x|))^2.
 *   Every element is formed in float64 and rounded to f32 once.  Two launches: workgroup b owns elements [b E, (b + 1) E),
 *   E = 256 ceil(M / 2^16), thread t adding the elements b E + t, + 256, .. in ascending order and the 256 threads by
 *   block_sum's order, into float64 partials (BCE, I, S) in ws; then every workgroup re-sums the partials in ascending order and
 *   writes its elements, workgroup 0 the loss.  ws: lnh_unet_loss_grad_workspace_size(M) = ceil(M / E) x 24 bytes (0: refused M).
 * lnh_urs_tensor / the table: n_tensors (1 .. LNH_URS_MAX_TENSORS) records IN DEVICE MEMORY, one per parameter tensor.  The entry
 *   points cannot read it, so its contents are the caller's to guarantee: valid 4-byte aligned pointers to numel f32 each
 *   (momentum_buffer may be NULL only for momentum == 0), numel at most 2^40 per tensor (0 is allowed: the record is passed over)
 *   and fewer than 2^32 chunks of 4096 elements in the whole table — chunk counts are kept in 32 bits and wrap beyond that.
 * state: LNH_URS_SLOTS doubles in device memory (the slots below).
 * lnh_unet_grad_sumsq: state[LNH_URS_SUMSQ] = the sum of grad^2 over all elements of all tensors of the table in float64, and
 *   state[LNH_URS_NONFINITE] = 1 if that sum is not finite — i.e. if any element is inf or NaN: squares cannot cancel and cannot
 *   overflow a float64 — else 0.  A tensor is cut into chunks of 4096 elements; workgroup b of 1024 takes chunks b, b + 1024, .. of
 *   the table's chunk list in ascending order; within a chunk thread t owns elements 4 q .. 4 q + 3 for q = t, t + 256, t + 512,
 *   t + 768, ascending (read as float4 where the tensor starts on 16 bytes, as scalars otherwise: the same order); the threads are
 *   added by block_sum's order and the 1024 partials in ascending order.  ws: lnh_unet_grad_sumsq_workspace_size() = 8192 bytes.
 * lnh_unet_rmsprop_step: clip_grad_norm_(max_norm) on the unscaled gradients + torch.optim.RMSprop(foreach=True) for every
 *   tensor of the table in ONE launch, from state[LNH_URS_SUMSQ] / [LNH_URS_NONFINITE] (lnh_unet_grad_sumsq's) and the learning
 *   rate state[LNH_URS_LR], read on the device.  norm = sqrt(sumsq) / loss_scale and coef = min(1, max_norm / (norm + 1e-6)) in
 *   float64; then per element in fp32, every operation rounded on its own: g = grad (1 / loss_scale); g = g coef; g = g + wd p
 *   (if wd != 0); sq = sq alpha; sq = sq + ((1 - alpha) g) g; avg = sqrt(sq) + eps; buf = buf momentum; buf = buf + g / avg;
 *   p = p + (-lr) buf (momentum == 0: p = p + (-lr) (g / avg), momentum_buffer not touched).  Writes state[LNH_URS_NORM],
 *   [LNH_URS_COEF] and adds 1 to [LNH_URS_STEP].  With state[LNH_URS_NONFINITE] != 0 the step is skipped as GradScaler.step skips
 *   it: no tensor is written, [LNH_URS_SKIPPED] goes up by 1 and [LNH_URS_STEP] stays.  The gradients are never written. */
#define LNH_UNET_MASK_F32 0u
#define LNH_UNET_MASK_U8 1u
#define LNH_URS_MAX_TENSORS 64
#define LNH_URS_LR 0        /* learning rate: written by the caller (a scheduler), read by every step */
#define LNH_URS_STEP 1      /* steps taken */
#define LNH_URS_SKIPPED 2   /* steps skipped for a non-finite gradient */
#define LNH_URS_SUMSQ 3     /* the last sum of squares of the (scaled) gradients */
#define LNH_URS_NORM 4      /* the last total norm of the unscaled gradients */
#define LNH_URS_COEF 5      /* the last clip coefficient, as the f32 every element was multiplied by */
#define LNH_URS_NONFINITE 6 /* 1 if the last sum of squares was not finite */
#define LNH_URS_SLOTS 8
typedef struct lnh_urs_tensor {
    float *param;
    const float *grad;
    float *square_avg;
    float *momentum_buffer;
    uint64_t numel;
} lnh_urs_tensor;
LNH_API uint64_t lnh_unet_loss_grad_workspace_size(uint64_t M);
LNH_API int lnh_unet_loss_grad(const float *logits, const void *masks, uint32_t mask_dtype, uint64_t M, double loss_scale, void *ws,
                               uint64_t ws_bytes, float *loss, float *dlogits, lnh_stream_t stream);
LNH_API uint64_t lnh_unet_grad_sumsq_workspace_size(void);
LNH_API int lnh_unet_grad_sumsq(const lnh_urs_tensor *table, uint32_t n_tensors, void *ws, uint64_t ws_bytes, double *state,
                                lnh_stream_t stream);
LNH_API int lnh_unet_rmsprop_step(const lnh_urs_tensor *table, uint32_t n_tensors, double *state, double loss_scale, double max_norm,
                                  double alpha, double eps, double weight_decay, double momentum, lnh_stream_t stream);

/* ---- evaluation: nearest-neighbour pass of the chamfer distance (extern/chamfer3D/chamfer3D.cu:9-138)
 * dist[j] = min_k |xyz1[j] - xyz2[k]|^2 (squared), idx[j] = the first k attaining it; xyz* are [n,3] / [m,3] f32.
 */
LNH_API int lnh_chamfer_nn(const float *xyz1, uint32_t n, const float *xyz2, uint32_t m, float *dist, int32_t *idx,
                           lnh_stream_t stream);

/* ---- optimizer step of the hash table (nerf/utils.py:1206-1226: GradScaler + torch.optim.Adam, fused) ------------
 * lnh_grad_check_f16: *found_inf = 1 if any of the n fp16 gradient values is inf / nan (never clears it).
 * lnh_adam_table_step: torch.optim.Adam (no weight decay / amsgrad) on fp32 param / exp_avg / exp_avg_sq with the
 *   fp16 gradient scaled by *inv_scale; also writes the fp16 copy of the updated parameters.  *found_inf != 0 skips
 *   the whole update.  The step counter t lives on the device, double-buffered: reads *step_in, writes *step_out.
 * lnh_adam_table_step_dlr: the same with the learning rate read from device memory (*lr, f32) — for a training step
 *   captured in a hipGraph, whose kernel arguments are frozen at capture while the schedule moves lr every step
 *   (main_lidarnerf.py:408-410: LambdaLR).
 */
LNH_API int lnh_grad_check_f16(const void *grad16, uint64_t n, float *found_inf, lnh_stream_t stream);
LNH_API int lnh_adam_table_step(float *param, float *exp_avg, float *exp_avg_sq, const void *grad16, void *param16,
                                uint64_t n, double lr, double beta1, double beta2, double eps,
                                const float *inv_scale, const float *found_inf, const float *step_in,
                                float *step_out, lnh_stream_t stream);
LNH_API int lnh_adam_table_step_dlr(float *param, float *exp_avg, float *exp_avg_sq, const void *grad16, void *param16,
                                    uint64_t n, const float *lr, double beta1, double beta2, double eps,
                                    const float *inv_scale, const float *found_inf, const float *step_in,
                                    float *step_out, lnh_stream_t stream);

/* ---- the whole optimizer step of a training iteration as two launches (nerf/utils.py:1216-1226: scaler.step(optimizer),
 * scaler.update(), lr_scheduler.step(); main_lidarnerf.py:389-391, 408-410: Adam(betas .9/.99, eps 1e-15), lr0 * 0.1^(it/iters))
 * The scalars of the step live in ONE device buffer `state` of LNH_TRAIN_STATE_FLOATS floats (indices LNH_TS_*), so a
 * training step captured in a hipGraph needs no host value:
 *   SCALE / GROWTH   GradScaler's loss scale and growth counter          T / T_NEXT     Adam's step count, before / after
 *   FOUND            stamp IT + 1 of the last step that saw an inf/nan   IT / IT_NEXT   scheduler steps taken, before / after
 *   INV / INV_TABLE  1 / (scale * div_small), 1 / (scale * div_table)    LR             lr0 * 0.1^min(IT / iters, 1)
 *   LAST_SCALE       the scale the gradients of the last step carry      SKIPPED        1 if the last step was skipped
 * lnh_train_check: commits T_NEXT / IT_NEXT of the previous step, forms INV / INV_TABLE / LAST_SCALE / LR, and stamps
 *   FOUND = IT + 1 if the n16 fp16 values at grad16 or any of the small fp32 gradients holds an inf / nan (idempotent:
 *   may be called once per piece of a gradient that arrives in pieces; a MAX all-reduce of FOUND over ranks keeps the
 *   stamp).  div_table / div_small = what the SUMMED gradients still have to be divided by (data parallel: the world size).
 * lnh_train_step: Adam with torch's fused arithmetic on the fp32 table (n values, fp16 gradient, also writes the fp16
 *   copy; n = 0: the table is stepped elsewhere, e.g. lnh_adam_table_step_dlr per shard with lr = &state[LNH_TS_LR],
 *   inv_scale = &state[LNH_TS_INV_TABLE], found_inf = &state[LNH_TS_SKIPPED], step_in / step_out = &state[LNH_TS_T] /
 *   &state[LNH_TS_T_NEXT]) and on n_small <= LNH_TRAIN_MAX_SMALL fp32 tensors (host arrays of device pointers; a null
 *   gradient skips that tensor; their moments lie back to back in small_exp_avg / small_exp_avg_sq in the order given),
 *   skipped as a whole when FOUND == IT + 1; then T_NEXT, IT_NEXT, SKIPPED and torch's amp_update_scale_.
 * lnh_zero_regions: clears up to 8 device regions (host arrays of pointers and byte counts, 4-byte granular) with ONE launch.
 */
#define LNH_TRAIN_STATE_FLOATS 16
#define LNH_TRAIN_MAX_SMALL 16
#define LNH_TS_SCALE 0
#define LNH_TS_GROWTH 1
#define LNH_TS_FOUND 2
#define LNH_TS_INV 3
#define LNH_TS_INV_TABLE 4
#define LNH_TS_LAST_SCALE 5
#define LNH_TS_T 6
#define LNH_TS_IT 7
#define LNH_TS_LR 8
#define LNH_TS_T_NEXT 9
#define LNH_TS_IT_NEXT 10
#define LNH_TS_SKIPPED 11
LNH_API int lnh_train_check(float *state, const void *grad16, uint64_t n16, const float *const *small_grads,
                            const uint32_t *small_numel, uint32_t n_small, float div_table, float div_small, double lr0,
                            double iters, lnh_stream_t stream);
LNH_API int lnh_train_step(float *state, float *param, float *exp_avg, float *exp_avg_sq, const void *grad16,
                           void *param16, uint64_t n, float *const *small_params, const float *const *small_grads,
                           const uint32_t *small_numel, uint32_t n_small, float *small_exp_avg, float *small_exp_avg_sq,
                           double beta1, double beta2, double eps, double growth_factor, double backoff_factor,
                           uint32_t growth_interval, lnh_stream_t stream);
LNH_API int lnh_zero_regions(void *const *ptrs, const uint64_t *bytes, uint32_t count, lnh_stream_t stream);

/* ---- exponential moving average of the parameters (nerf/utils.py:619-624, 1257-1258, 1297-1299, 1444-1445: torch_ema's
 * ExponentialMovingAverage over model.parameters(), update() per epoch, the averaged weights swapped in for evaluation).
 * Like lnh_train_step ONE launch covers the fp32 table (n values; n = 0: no table, its pointers may be null) and
 * n_small <= LNH_TRAIN_MAX_SMALL fp32 tensors (host arrays of device pointers and element counts, 4-byte aligned).
 * lnh_ema_update: for every element, in fp32, three separately rounded operations in torch_ema's order:
 *   tmp = shadow - param;  tmp = tmp * one_minus_decay;  shadow = shadow - tmp
 *   — bit-identical to those three torch operations on fp32 tensors (no fused multiply-add).  one_minus_decay in [0, 1] is
 *   formed by the host (torch_ema: 1 - min(decay, (1 + num_updates) / (10 + num_updates)) in double, then rounded to float).
 * lnh_ema_swap: exchanges param and shadow in place; for the table it also writes param16[i] = (half)param_new[i] in the
 *   same pass (param16 null: no fp16 compute copy is kept).  Applied twice it is the identity, bit for bit: it replaces
 *   torch_ema's store() + copy_to() before an evaluation and restore() after it without a third copy of the parameters.
 * Table buffers: 16-byte (fp32) / 8-byte (fp16) aligned; param and shadow must not alias.
 */
LNH_API int lnh_ema_update(float *shadow, const float *param, uint64_t n, float *const *small_shadow,
                           const float *const *small_param, const uint32_t *small_numel, uint32_t n_small,
                           float one_minus_decay, lnh_stream_t stream);
LNH_API int lnh_ema_swap(float *param, float *shadow, void *param16, uint64_t n, float *const *small_param,
                         float *const *small_shadow, const uint32_t *small_numel, uint32_t n_small, lnh_stream_t stream);

/* ---- evaluation of one LiDAR frame (nerf/utils.py:886-1009 Trainer.eval_step / test_step after model.render, and what
 * evaluate_one_epoch's meters compute from the returned images, 1357-1366 with MAEMeter / RMSEMeter / DepthMeter, 226-362),
 * on the caller's stream, with no host read between the rendered outputs and the accumulated numbers.  (Added without
 * moving lnh_version: detect the entry points by symbol.)
 * Inputs: image_lidar [H*W, 2] (ray-drop, intensity) and depth_lidar [H*W] as the renderer returns them (f32), gt [H, W, 3]
 * (ray-drop, intensity, depth).  Of `options` only depth_loss / raydrop_loss / intensity_loss (LNH_LOSS_L1 .. LNH_LOSS_BCE;
 * LNH_LOSS_COS is a patch criterion and is refused), huber_delta, alpha_d / alpha_r / alpha_i and scale are read.
 * Rules, with the reference's lines:
 *   - mask = image_lidar[:, 0] > 0.5 (930 / 1002); LNH_EVAL_MODE_EVAL multiplies predicted intensity and depth by it only
 *     if alpha_r > 0 and some pixel of the mask is set (936-938), LNH_EVAL_MODE_TEST whenever alpha_r > 0 (1005-1007).
 *   - ground-truth intensity and depth are multiplied by the ground-truth ray-drop before anything is compared (913-914).
 *   - nerf_mvl: ground-truth ray-drop -1 marks pixels outside the sensor's window (902-911): zeroed in the ground truth,
 *     removed from the mask in EVAL mode (931-932; test_step has no ground truth and keeps them); the loss is still the mean
 *     over the whole frame (940-946); the intensity meters and DepthMeter see the valid pixels (948-956, 1357-1366), which
 *     the reference requires to fill their bounding rectangle — slots CROP_* and VALID let the host check that.
 *   - loss = alpha_d mean C_depth(pred_depth, gt_depth) + alpha_r mean C_raydrop(pred_raydrop, gt_raydrop) + alpha_i mean
 *     C_intensity(pred_intensity, gt_intensity) on the masked images (940-946).
 *   - MAEMeter: mean |gt_i inv_scale - pred_i inv_scale| (290-292); RMSEMeter: sqrt(mean (gt_i - pred_i)^2) (249-250), both
 *     on the INTENSITY images (1358-1359); DepthMeter (328-360): both depth images / scale, clamped to [1e-3, 80] m, rmse,
 *     a_k = mean(max(gt/pred, pred/gt) < 1.25^k), SSIM with data_range = max - min of the clamped ground truth.
 * lnh_lidar_eval_frame: writes the images eval_step / test_step return — pred_intensity, pred_depth [H*W] (masked as above)
 *   and pred_mask [H*W] (1.0 / 0.0: the thresholded ray-drop, in EVAL mode times the valid window) — and leaves per-workgroup
 *   partial sums in the workspace.  gt == NULL (LNH_EVAL_MODE_TEST only): the three images alone, H, W >= 1, no workspace.
 * lnh_lidar_eval_ssim: mean SSIM of pred_depth (lnh_lidar_eval_frame's output) against the ground-truth depth, both / scale
 *   and clamped, with skimage.metrics.structural_similarity's defaults (uniform 7x7 window, sample covariance, K1 0.01, K2
 *   0.03, mean over the windows the image covers completely), window moments in fp64; over the bounding rectangle of the
 *   valid pixels with nerf_mvl; data_range is read from the partials lnh_lidar_eval_frame left.  Leaves its partial sums
 *   in the workspace.  A rectangle smaller than 7 x 7 gives NaN (and a frame without a valid pixel NaN in every meter
 *   slot): such a row is added like any other, so the accumulator's means become NaN — slot LNH_EVAL_BAD counts these
 *   frames, and a caller must not report the means of an accumulator whose LNH_EVAL_BAD is not 0.
 * lnh_lidar_eval_finalize: adds the partials in index order, forms the frame's row of LNH_EVAL_SLOTS doubles, stores it at
 *   history[frame * LNH_EVAL_SLOTS] when frame = accumulator[LNH_EVAL_FRAMES] < max_frames (history may be NULL with
 *   max_frames 0), and adds it to accumulator[LNH_EVAL_SLOTS] (clear that before the first frame): meters are means of
 *   per-frame values (252-256, 362-364), i.e. accumulator[slot] / accumulator[LNH_EVAL_FRAMES].
 * Call the three in this order on one stream with the same H, W, mode, nerf_mvl and workspace
 * (lnh_lidar_eval_workspace_bytes(H, W) bytes, 8-byte aligned, contents irrelevant; 0 for an unsupported shape).
 * Deterministic (fixed-order sums, no float atomics); no allocation, copy or synchronisation: capturable in a hipGraph.
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null pointer, H or W < 7, an unknown mode or criterion, COS, scale
 * <= 0, a workspace smaller than the query; LNH_ERR_UNSUPPORTED for more than 2^24 pixels.
 */
enum { LNH_EVAL_MODE_EVAL = 0, LNH_EVAL_MODE_TEST = 1 };
enum {
    LNH_EVAL_LOSS = 0,           /* validation loss of the frame */
    LNH_EVAL_LOSS_DEPTH = 1,     /* its three unweighted terms (means of the criteria) */
    LNH_EVAL_LOSS_RAYDROP = 2,
    LNH_EVAL_LOSS_INTENSITY = 3,
    LNH_EVAL_MAE = 4,            /* MAEMeter on the intensity images */
    LNH_EVAL_RMSE = 5,           /* RMSEMeter on the intensity images */
    LNH_EVAL_DEPTH_RMSE = 6,     /* DepthMeter: rmse [m], a1, a2, a3, ssim */
    LNH_EVAL_A1 = 7,
    LNH_EVAL_A2 = 8,
    LNH_EVAL_A3 = 9,
    LNH_EVAL_SSIM = 10,
    LNH_EVAL_MASKED = 11,        /* 1 if the ray-drop mask was applied to intensity and depth */
    LNH_EVAL_CROP_R0 = 12,       /* bounding rectangle of the valid pixels: first row, first column, height, width */
    LNH_EVAL_CROP_C0 = 13,
    LNH_EVAL_CROP_H = 14,
    LNH_EVAL_CROP_W = 15,
    LNH_EVAL_VALID = 16,         /* number of valid pixels (== CROP_H * CROP_W for a rectangular window) */
    LNH_EVAL_DATA_RANGE = 17,    /* max - min of the clamped ground-truth depth [m] */
    LNH_EVAL_FRAMES = 18,        /* 1 per row: the accumulator's frame count */
    LNH_EVAL_BAD = 19,           /* 1 if the means cannot use the row: a non-finite number, or valid pixels that do not fill
                                    their rectangle; the accumulator counts such frames and the host refuses them */
    LNH_EVAL_SLOTS = 20
};
LNH_API uint64_t lnh_lidar_eval_workspace_bytes(uint32_t H, uint32_t W);
LNH_API int lnh_lidar_eval_frame(const float *image_lidar, const float *depth_lidar, const float *gt, uint32_t H, uint32_t W,
                                 const lnh_lidar_loss_options *options, float intensity_inv_scale, int32_t mode,
                                 int32_t nerf_mvl, void *workspace, uint64_t workspace_bytes, float *pred_intensity,
                                 float *pred_depth, float *pred_mask, lnh_stream_t stream);
LNH_API int lnh_lidar_eval_ssim(const float *pred_depth, const float *gt, uint32_t H, uint32_t W, float scale,
                                int32_t nerf_mvl, void *workspace, uint64_t workspace_bytes, lnh_stream_t stream);
LNH_API int lnh_lidar_eval_finalize(uint32_t H, uint32_t W, const lnh_lidar_loss_options *options, int32_t mode,
                                    int32_t nerf_mvl, const void *workspace, uint64_t workspace_bytes, double *accumulator,
                                    double *history, uint32_t max_frames, lnh_stream_t stream);

/* ---- points meter of one evaluation frame (nerf/utils.py:375-427 PointsMeter: both range images back-projected to point
 * clouds, extern/chamfer3D's nearest-neighbour distances between them, extern/fscore.py), from two depth images to a row of
 * numbers on the device, on the caller's stream, with no host read.  (Added without moving lnh_version: detect by symbol.)
 * Buffers of the caller, capacity = H * W: cloud_pred / cloud_gt [capacity, 4] f32 (x, y, z, 0; 16-byte aligned), counts
 * uint32[2] (points of cloud_pred, cloud_gt), dist_* [capacity] f32, idx_* [capacity] int32; one workspace of
 * lnh_eval_points_workspace_bytes(H, W) bytes (16-byte aligned, contents irrelevant; 0 for an unsupported shape).
 * lnh_eval_points_project: pred_depth [H*W] (the masked depth lnh_lidar_eval_frame writes) and gt [H, W, 3] (ray-drop,
 *   intensity, depth; with nerf_mvl a ray-drop of -1 counts as 0) -> the metric depth images pred * (1 / scale) and
 *   gt_depth * gt_raydrop * (1 / scale) (torch's tensor / host scalar: a product with the float32 reciprocal), every pixel
 *   back-projected with lnh_pano_to_lidar's arithmetic, the pixels with depth != 0 compacted in row-major pixel order into
 *   the two clouds, and the two counts.  Rows >= count are left as they were.  Equal, bit for bit and row for row, to
 *   convert.pano_to_lidar(depth / scale, (fov_up, fov)).
 * lnh_eval_points_nn: for every point of each cloud the SQUARED distance to, and the index of, its nearest point in the
 *   other cloud (first index on ties), both directions in one call, counts read from device memory: dist_pred / idx_pred
 *   [counts[0]] against cloud_gt, dist_gt / idx_gt [counts[1]] against cloud_pred — bit-identical to two lnh_chamfer_nn
 *   calls.  Rows >= count of the clouds are never read.  An empty target cloud gives +inf / 0.
 * lnh_eval_points_finalize: sums both distance arrays in a fixed order in fp64, counts dist < threshold on each side, forms
 *   the row of LNH_PTS_SLOTS doubles, stores it at history[frame * LNH_PTS_SLOTS] when frame = accumulator[LNH_PTS_FRAMES] <
 *   max_frames (history may be NULL with max_frames 0) and adds it to accumulator[LNH_PTS_SLOTS] (clear that before the
 *   first frame): the meter is the mean of per-frame values, accumulator[slot] / accumulator[LNH_PTS_FRAMES].  A frame with
 *   an empty cloud on either side has no chamfer distance: its row holds NaN, the distance arrays are not read, and
 *   LNH_PTS_BAD counts it — a caller must not report the means of an accumulator whose LNH_PTS_BAD is not 0.
 * Call the three in this order on one stream.  Deterministic (integer minimum over the partial searches, fixed-order sums, no
 * float atomics); no allocation, copy or synchronisation: capturable in a hipGraph.
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null or misaligned pointer, H * W = 0, scale or threshold <= 0, a
 * workspace smaller than the query; LNH_ERR_UNSUPPORTED for more than 2^24 pixels.
 */
enum {
    LNH_PTS_CHAMFER = 0,     /* mean(dist_pred) + mean(dist_gt) */
    LNH_PTS_FSCORE = 1,      /* 2 p r / (p + r), 0 where that is NaN (extern/fscore.py) */
    LNH_PTS_PRECISION = 2,   /* p: share of dist_pred < threshold */
    LNH_PTS_RECALL = 3,      /* r: share of dist_gt < threshold */
    LNH_PTS_MEAN_PRED = 4,   /* the two means */
    LNH_PTS_MEAN_GT = 5,
    LNH_PTS_COUNT_PRED = 6,  /* the two point counts */
    LNH_PTS_COUNT_GT = 7,
    LNH_PTS_FRAMES = 8,      /* 1 per row: the accumulator's frame count */
    LNH_PTS_BAD = 9,         /* 1 if the means cannot use the row: an empty cloud or a non-finite chamfer distance */
    LNH_PTS_SLOTS = 10
};
LNH_API uint64_t lnh_eval_points_workspace_bytes(uint32_t H, uint32_t W);
LNH_API int lnh_eval_points_project(const float *pred_depth, const float *gt, uint32_t H, uint32_t W, float fov_up, float fov,
                                    float scale, int32_t nerf_mvl, void *workspace, uint64_t workspace_bytes,
                                    float *cloud_pred, float *cloud_gt, uint32_t *counts, lnh_stream_t stream);
LNH_API int lnh_eval_points_nn(const float *cloud_pred, const float *cloud_gt, const uint32_t *counts, uint32_t capacity,
                               void *workspace, uint64_t workspace_bytes, float *dist_pred, int32_t *idx_pred,
                               float *dist_gt, int32_t *idx_gt, lnh_stream_t stream);
LNH_API int lnh_eval_points_finalize(const float *dist_pred, const float *dist_gt, const uint32_t *counts, uint32_t capacity,
                                     float threshold, double *accumulator, double *history, uint32_t max_frames,
                                     lnh_stream_t stream);

/* ---- meters of the NVS baselines' evaluation (lidarnvs/eval.py:9-135 eval_points_and_pano, after the NeRF-MVL crop of
 * lidarnvs/run.py:200-217), from four images of one frame to a row of numbers on the device, on the caller's stream, with no
 * host read.  (Added without moving lnh_version: detect by symbol.)  NOT the trainer's meters (lnh_lidar_eval_*): images are
 * in world scale and flattened first, so the SSIM is 1-D with a 7-wide window over the row-major sequence; dropped pixels
 * (depth 0) take part in the depth metrics, clamped to 1e-3; there is no ray-drop masking.
 * gt_pano, pd_pano, gt_int, pd_int: [H*W] f32; mask: [H*W] uint8 or NULL for "every pixel".  The evaluated sequence is the
 * pixels with mask != 0 in row-major order, n of them; it is addressed as their bounding rectangle of h x w pixels at
 * (r0, c0), element p at (r0 + p / w, c0 + p % w): the reference's reshape to (h, w) needs n == h * w, and a frame where
 * that fails is marked bad.  One workspace of lnh_nvs_eval_workspace_bytes(H, W) bytes (8-byte aligned, contents irrelevant;
 * 0 for an unsupported shape) carries the partials from call to call.
 * lnh_nvs_eval_frame: per element, in float32 and in the reference's operation order: both depths clamped to [1e-3, 80]
 *   (a NaN stays a NaN), thresh = max(gt / pd, pd / gt), the three strict comparisons thresh < 1.25, < 1.5625, < 1.953125,
 *   (gt - pd)^2, |gt_i * intensity_scale - pd_i * intensity_scale| (intensity_scale: 1 for KITTI-360, 255 for NeRF-MVL).
 *   Per workgroup: the counts and the rectangle as integers, the two sums in fp64, min / max of the clamped ground truth.
 * lnh_nvs_eval_ssim: skimage.metrics.structural_similarity's defaults on the two clamped sequences as 1-D signals: uniform
 *   window of 7, sample covariance (7 / 6), K1 0.01, K2 0.03, data_range = the float32 max - min of the clamped ground
 *   truth, the mean over the n - 6 positions whose window lies inside the sequence.  The five window moments are fp64 sums of
 *   the 7 float32 values from left to right, S is formed in fp64 with one rounded operation per operator (two identical
 *   images give exactly 1).  `mask` is the one lnh_nvs_eval_frame was given; it is not read (the rectangle comes from the
 *   partials).  Over the rectangle also where the masked pixels do not fill it (that frame is bad).
 * lnh_nvs_eval_finalize: adds the partials in index order, forms the frame's row of LNH_NVS_SLOTS doubles — chamfer and
 *   F-score copied from points_row, the LNH_PTS_* row lnh_eval_points_finalize made for the same frame (a device pointer) —
 *   stores it at history[frame * LNH_NVS_SLOTS] when frame = accumulator[LNH_NVS_FRAMES] < max_frames (history may be NULL
 *   with max_frames 0) and adds it to accumulator[LNH_NVS_SLOTS] (clear that before the first frame): the meters are means
 *   of per-frame values.  n < 7 gives an SSIM of NaN; data_range 0 is not special-cased (the IEEE result stands).
 * Call the three in this order on one stream.  Deterministic (integer atomics in LDS only, fixed-order fp64 sums); no
 * allocation, copy or synchronisation: capturable in a hipGraph.
 * Errors (before any launch): LNH_ERR_INVALID_ARG for a null or misaligned pointer, H * W = 0, an intensity_scale that is not
 * positive and finite, a workspace smaller than the query; LNH_ERR_UNSUPPORTED for more than 2^24 pixels.
 */
enum {
    LNH_NVS_DEPTH_RMSE = 0,    /* sqrt(sum (gt - pd)^2 / n) */
    LNH_NVS_DEPTH_A1 = 1,      /* share of thresh < 1.25, 1.25^2, 1.25^3 */
    LNH_NVS_DEPTH_A2 = 2,
    LNH_NVS_DEPTH_A3 = 3,
    LNH_NVS_DEPTH_SSIM = 4,    /* mean 1-D SSIM */
    LNH_NVS_INTENSITY_MAE = 5, /* sum |gt_i s - pd_i s| / n */
    LNH_NVS_CHAMFER = 6,       /* points_row[LNH_PTS_CHAMFER] */
    LNH_NVS_FSCORE = 7,        /* points_row[LNH_PTS_FSCORE] */
    LNH_NVS_CROP_R0 = 8,       /* the bounding rectangle of the masked pixels (0 0 0 0 for an empty mask) */
    LNH_NVS_CROP_C0 = 9,
    LNH_NVS_CROP_H = 10,
    LNH_NVS_CROP_W = 11,
    LNH_NVS_N = 12,            /* masked pixels */
    LNH_NVS_DATA_RANGE = 13,   /* of the clamped ground truth (NaN for an empty mask) */
    LNH_NVS_SUM_SQ = 14,       /* the two fp64 sums the rmse and the mae are made of */
    LNH_NVS_SUM_ABS = 15,
    LNH_NVS_FRAMES = 16,       /* 1 per row: the accumulator's frame count */
    LNH_NVS_BAD = 17,          /* 1 if the means cannot use the row: a non-finite metric, n < 7, an empty mask, masked pixels
                                  that do not fill their rectangle, or a bad points row */
    LNH_NVS_SLOTS = 18
};
LNH_API uint64_t lnh_nvs_eval_workspace_bytes(uint32_t H, uint32_t W);
LNH_API int lnh_nvs_eval_frame(const float *gt_pano, const float *pd_pano, const float *gt_int, const float *pd_int,
                               const uint8_t *mask, uint32_t H, uint32_t W, float intensity_scale, void *workspace,
                               uint64_t workspace_bytes, lnh_stream_t stream);
LNH_API int lnh_nvs_eval_ssim(const float *gt_pano, const float *pd_pano, const uint8_t *mask, uint32_t H, uint32_t W,
                              void *workspace, uint64_t workspace_bytes, lnh_stream_t stream);
LNH_API int lnh_nvs_eval_finalize(uint32_t H, uint32_t W, const void *workspace, uint64_t workspace_bytes,
                                  const double *points_row, double *accumulator, double *history, uint32_t max_frames,
                                  lnh_stream_t stream);

/* ------------------------------------------------------------------ training batches drawn on the device ----- */
/*
 * Replaces KITTI360Dataset.collate / NeRFMVLDataset.collate + get_lidar_rays for a sequence that is preloaded on the
 * device (lidarnerf/dataset/base_dataset.py:16-105, kitti360_dataset.py:123-159): one launch of one thread per ray draws
 * the batch of a training step, a second one-thread launch moves the cursor on.  No atomics, no host synchronisation,
 * and nothing that changes from step to step is a kernel argument — a captured launch draws a fresh batch per replay.
 * poses [F,4,4] f32 (lidar -> world, row-major); images [F,H,W,3] of image_dtype (LNH_F32 / LNH_F16); (fov_up, fov) in
 * degrees; perm [F] int32, the frame order of the epoch (an entry is taken modulo F; may be NULL with an explicit frame);
 * cursor [2] uint64: [0] the step within the epoch, [1] the number of draws since the sampler was made (never reset);
 * (seed_lo, seed_hi) the 64-bit seed; stream_id >= 0 the data-parallel rank; frame = -1: perm[cursor[0] % F], else that
 * frame.  Rows written, n (base_dataset.py:45-52, quirks included): px > 0: (min(n_rays, H*W) / (px*py)) * px*py — patches
 * of px rows x py columns, row-major inside a patch, top-left corners uniform over [0, H-px) x [0, W-py) (the last row and
 * column are never drawn); px <= 0: min(n_rays, H*W) independent pixels over H*W (py is ignored).
 * Outputs: rays_o, rays_d [n,3] f32 (rays_o = the pose's translation, rays_d = R * (cos a cos b, cos a sin b, sin a) with
 * b = -(col - W/2)/W * 2 pi, a = (fov_up - row/H * fov) * pi/180); gt [n,3] of image_dtype (the pixel's three values, bit
 * for bit); inds [n] int32 = row * W + col.  After the draw both cursor entries are incremented (also when n == 0).
 * Randomness: Philox-4x32-10, key (seed_lo, seed_hi), counter (patch index — ray index with px <= 0 —, cursor[1] low,
 * cursor[1] high, stream_id); word 0 -> row (or the flat pixel), word 1 -> column; a word r maps to [0, m) as
 * (uint64(r) * m) >> 32.  Not torch's randint stream.
 * Refused (LNH_ERR_INVALID_ARG, the message names the argument): F <= 0, n_rays <= 0, px > 0 with py <= 0, px >= H or
 * py >= W (the reference's randint(0, 0) raises too), a frame outside [-1, F), stream_id < 0, a NULL pointer;
 * LNH_ERR_UNSUPPORTED: H*W > 2^24, another image_dtype.
 */
LNH_API int lnh_lidar_sample_batch(const float *poses, const void *images, int image_dtype, int32_t F, uint32_t H, uint32_t W,
                                   float fov_up, float fov, const int32_t *perm, uint64_t *cursor, uint32_t seed_lo,
                                   uint32_t seed_hi, int32_t stream_id, int32_t n_rays, int32_t px, int32_t py,
                                   int32_t frame, float *rays_o, float *rays_d, void *gt, int32_t *inds,
                                   lnh_stream_t stream);
/* Every pixel of one frame, for evaluation: rays_o, rays_d [H*W,3] f32 of poses[frame] (a HOST index in [0, F)), the same
 * arithmetic as above.  No randomness, no cursor. */
LNH_API int lnh_lidar_frame_rays(const float *poses, int32_t F, int32_t frame, uint32_t H, uint32_t W, float fov_up,
                                 float fov, float *rays_o, float *rays_d, lnh_stream_t stream);


/* ------------------------------------------------------------------ bf16 MLP operands (BASELINE config 5) ---- */
/*
 * The same eleven entry points with v_mfma_f32_16x16x32_bf16 operands ("fp16 hash features + bf16 MFMA MLP"; the
 * reference reaches the MLPs through torch.autocast, lidarnerf/nerf/utils.py:626,1212 — under
 * autocast(dtype=torch.bfloat16) its Linear stacks run in bf16 while the grid encoder keeps casting its table to half,
 * gridencoder/grid.py:54-57).  Every buffer that holds MLP-side 16-bit data is bf16 here — inputs / outputs /
 * forward_buffer / grad / grad_inputs of lnh_mlp_*_bf16, the packed weights, h16 and grad_h16 — while the hash-grid
 * `features` entering lnh_density_mlp_forward_bf16 and the `grad_features` leaving lnh_density_mlp_backward_bf16 stay
 * fp16 (the grid kernels' type).  Accumulation is fp32, weight gradients are fp32, as in the fp16 build.
 */
LNH_API int lnh_mlp_forward_bf16(const void *inputs, const void *weights, uint32_t B, uint32_t input_dim,
                            uint32_t output_dim, uint32_t hidden_dim, uint32_t n_hidden_mats, uint32_t activation,
                            uint32_t output_activation, void *forward_buffer, void *outputs, lnh_stream_t stream);
LNH_API int lnh_mlp_backward_bf16(const void *grad, const void *inputs, const void *weights, uint32_t B,
                             uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t n_hidden_mats,
                             uint32_t activation, uint32_t output_activation, void *grad_inputs, float *grad_weights,
                             void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
LNH_API int lnh_mlp_backward_data_bf16(const void *grad, const void *forward_buffer, const void *weights_t, uint32_t B,
                                       uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim,
                                       uint32_t n_hidden_mats, uint32_t activation, void *backward_buffer,
                                       void *grad_inputs, lnh_stream_t stream);
LNH_API int lnh_mlp_wgrad_bf16(const void *grad, const void *acts, uint32_t B, uint32_t M, uint32_t N, float *grad_weights,
                               void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
LNH_API int lnh_density_mlp_forward_bf16(const void *features, const void *weights, uint32_t B, uint32_t T_cur,
                                    uint32_t T_tot, uint32_t slot_off, uint32_t feat_rows, void *h16, float *sigma,
                                    lnh_stream_t stream);
LNH_API int lnh_density_mlp_backward_bf16(const void *grad_h16, const void *features, const void *weights, uint32_t B,
                                     uint32_t T_cur, uint32_t T_tot, uint32_t slot_off, void *grad_features,
                                     float *grad_weights, void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
LNH_API int lnh_ragged_pack_weights_bf16(const float *ws0, uint32_t ld_s0, const float *ws1, uint32_t ld_s1, const float *wc0,
                                         uint32_t ld_c0, uint32_t n_in, const float *wc1, uint32_t ld_c1, const float *wc2,
                                         uint32_t ld_c2, void *wsig16, void *wcol16, lnh_stream_t stream);
LNH_API int lnh_ragged_color_input_bf16(const float *dirs, const void *h16, uint32_t M, uint32_t degree, void *cin,
                                        lnh_stream_t stream);
LNH_API int lnh_ragged_color_input_rays_bf16(const float *dirs, const void *h16, const int32_t *rays, const float *deltas,
                                             uint32_t N, uint32_t M, uint32_t degree, void *cin, lnh_stream_t stream);
LNH_API int lnh_ragged_color_output_bf16(const void *y16, uint32_t M, float *rgb, lnh_stream_t stream);
LNH_API int lnh_ragged_color_output_backward_bf16(const float *grad_rgb, const float *rgb, uint32_t M, void *grad_y16,
                                                  lnh_stream_t stream);
LNH_API int lnh_ragged_grad_rows_bf16(const float *grad_sigma, float density_scale, const void *h16, const void *grad_cin,
                                      uint32_t degree, uint32_t M, void *grad_h16, lnh_stream_t stream);
LNH_API int lnh_lidar_dir_term_bf16(const float *dir_features, const float *w0, uint32_t ldw, uint32_t N, uint32_t K,
                               float *features16, float *cdir, lnh_stream_t stream);
LNH_API int lnh_lidar_dir_term_freq_bf16(const float *dirs, uint32_t degree, const float *w0, uint32_t ldw, uint32_t N,
                                         float *features16, float *cdir, lnh_stream_t stream);
LNH_API int lnh_lidar_pack_weights_bf16(const float *ws0, uint32_t ld_s0, const float *ws1, uint32_t ld_s1,
                                   const float *wc0, uint32_t ld_c0, uint32_t n_dir, const float *wc1, uint32_t ld_c1,
                                   const float *wc2, uint32_t ld_c2, void *wsig16, void *wcol16, lnh_stream_t stream);
LNH_API int lnh_lidar_step_prologue_bf16(const float *ws0, uint32_t ld_s0, const float *ws1, uint32_t ld_s1, const float *wc0,
                                         uint32_t ld_c0, uint32_t degree, const float *wc1, uint32_t ld_c1, const float *wc2,
                                         uint32_t ld_c2, void *wsig16, void *wcol16, const float *u, const float *rays_o,
                                         const float *rays_d, const float *aabb, float bound, uint32_t N, uint32_t T,
                                         uint32_t T_tot, float near, float far, float *z, float *x01, float *features16,
                                         float *cdir, lnh_stream_t stream);
LNH_API int lnh_ragged_color_forward_bf16(const void *h16, const int32_t *rays, const float *cdir, const void *w16, uint32_t N,
                                          uint32_t M, float *rgb, lnh_stream_t stream);
LNH_API int lnh_ragged_color_backward_bf16(const float *grad_rgb, const float *grad_sigma, float density_scale,
                                           const void *h16, const int32_t *rays, const float *cdir, const void *w16,
                                           uint32_t N, uint32_t M, void *grad_h16, float *grad_w, float *ray_sum,
                                           void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
LNH_API int lnh_lidar_color_forward_bf16(const void *h16, const int32_t *perm, const float *weights, const float *cdir,
                                    const void *w16, uint32_t N, uint32_t T, float *rgb, lnh_stream_t stream);
LNH_API int lnh_lidar_color_composite_forward_bf16(const float *z, const float *sigma_pt, const int32_t *perm,
                                                   const float *sample_dist, const void *h16, const float *cdir,
                                                   const void *w16, uint32_t N, uint32_t T, float density_scale,
                                                   float *sigma_m, float *weights, float *rgb, float *weights_sum,
                                                   float *depth, float *image, lnh_stream_t stream);
LNH_API int lnh_lidar_color_composite_forward_train_bf16(const float *z, const float *sigma_pt, const int32_t *perm,
                                                         const float *sample_dist, const void *h16, const float *cdir,
                                                         const void *w16, uint32_t N, uint32_t T, float density_scale,
                                                         const float *gt, float alpha_d, float alpha_r, float alpha_i,
                                                         const float *grad_scale, float *weights, float *weights_sum,
                                                         float *depth, float *image, float *grad_sigma,
                                                         float *grad_image, lnh_stream_t stream);
LNH_API int lnh_lidar_color_backward_bf16(const float *grad_rgb, const float *grad_sigma, const void *h16,
                                     const int32_t *perm, const float *weights, const float *cdir, const void *w16,
                                     uint32_t N, uint32_t T, void *grad_h16, float *grad_w, float *ray_sum,
                                     void *wgrad_ws, uint64_t wgrad_ws_bytes, lnh_stream_t stream);
LNH_API int lnh_lidar_color_backward_image_bf16(const float *grad_image, const float *grad_sigma, const void *h16,
                                                const int32_t *perm, const float *weights, const float *cdir,
                                                const void *w16, uint32_t N, uint32_t T, void *grad_h16,
                                                float *grad_w, float *ray_sum, void *wgrad_ws,
                                                uint64_t wgrad_ws_bytes, lnh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LIDARNERF_HIP_H */
