/*
 * ngp_hip.h -- C ABI of libngp_hip.so: the MI355X (gfx950) implementation of torch-ngp's instant-ngp
 * hot path (gridencoder, shencoder, raymarching, ffmlp).
 *
 * This is the drop-in boundary.  Each entry point replaces one callable of the reference's pybind
 * `_backend` modules (cited per function, paths relative to the reference checkout) and keeps its
 * argument order and meaning; the differences forced by a C ABI are uniform:
 *   - at::Tensor arguments become raw DEVICE pointers (the caller owns every buffer, exactly as in
 *     the reference where the Python wrapper allocates all outputs and workspaces);
 *   - at::optional<at::Tensor> becomes a pointer that may be NULL;
 *   - the element type that the reference dispatches on (AT_DISPATCH_FLOATING_TYPES_AND_HALF) is an
 *     explicit `dtype` code.  NGP_F64 is accepted by the grid encoder (forward, backward -- with a workspace --,
 *     total variation) and the SH encoder; the raymarching entries and the frequency encoder take float* and have
 *     *_f64 twins (the compositors, near_far_from_aabb, sph_from_ray, packbits; freq_encode forward / backward).
 *     Every other entry refuses fp64 with NGP_ERR_INVALID (the marchers, ffmlp, fused / graph / optimizer entries);
 *   - a trailing `stream` (a hipStream_t passed as void*; NULL = the legacy default stream the
 *     reference launches on);
 *   - every function returns 0 on success and a non-zero NGP_ERR_* code on failure, with a
 *     human-readable message available from ngp_last_error() (the Python binding turns it into the
 *     RuntimeError the reference's TORCH_CHECK / std::runtime_error would have produced).
 * No function allocates device memory, synchronises the device, or touches the host copy of any
 * buffer.  All launches are asynchronous on `stream`.
 *
 * Contracts kept from the reference: buffers the reference requires pre-zeroed stay caller-zeroed
 * (xyzs/dirs/deltas, grad_embeddings, grad_inputs of the grid and SH backward, grad_sigmas/grad_rgbs);
 * `counter` is read-modify-written.  (ffmlp_backward OVERWRITES grad_weights: no pre-zeroing needed.)
 */
#ifndef NGP_HIP_H
#define NGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ngp_stream_t; /* hipStream_t */

enum {
    NGP_OK = 0,
    NGP_ERR_INVALID = 1, /* bad argument (unsupported D/C/hidden_dim, NULL pointer, misaligned size) */
    NGP_ERR_LAUNCH = 2,  /* HIP reported a launch error */
    NGP_ERR_DEVICE = 3   /* no usable gfx950 device / runtime error */
};

enum { NGP_F32 = 0, NGP_F16 = 1, NGP_F64 = 2 };

#define NGP_MAX_LEVELS 32 /* grid encoder: L <= 32 */

/* message of the last failing call on the calling thread ("" if none) */
const char* ngp_last_error(void);
/* ABI version of this header (bumped on any signature change) */
int ngp_abi_version(void);
/* gfx architecture string the library was compiled for ("gfx950") */
const char* ngp_target_arch(void);

/* ---------------------------------------------------------------------------------------------
 * gridencoder      (reference: gridencoder/src/gridencoder.h:12-15, bindings.cpp:5-9)
 * --------------------------------------------------------------------------------------------- */

/* replaces grid_encode_forward (gridencoder.cu:448-471).
 * inputs [B,D] fp32 in [0,1]; embeddings [sO,C] dtype; offsets [L+1] int32 (device);
 * outputs [L,B,C] dtype; dy_dx [B,L*D*C] dtype or NULL.  D in {2,3,4,5}, C in {1,2,4,8}, L <= 32.
 * gridtype 0 = hash, 1 = tiled; interp 0 = linear, 1 = smoothstep.
 * NGP_F64: positions and interpolation weights as in the fp32 path (from the fp32 inputs), products with table
 * entries and their sums in fp64 (DESIGN.md "The fp64 path"). */
int ngp_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                            uint32_t gridtype, int align_corners, uint32_t interp, int dtype, ngp_stream_t stream);

/* replaces grid_encode_backward (gridencoder.cu:473-503).
 * grad [L,B,C] dtype; grad_embeddings [sO,C] dtype, pre-zeroed, accumulated with hardware atomics
 * (packed fp16 when dtype is F16 and C is even, as the reference); dy_dx / grad_inputs [B,D] dtype
 * both NULL or both non-NULL.  NGP_F64 needs scratch memory: use ngp_grid_encode_backward_ws (this
 * entry returns NGP_ERR_INVALID for it). */
int ngp_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                             void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                             uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners,
                             uint32_t interp, int dtype, ngp_stream_t stream);

/* replaces grad_total_variation (gridencoder.cu:639-645): inputs [B,D] dtype in [0,1]; adds into grad [sO,C].
 * NGP_F64: fp64 throughout, fp64 atomics. */
int ngp_grad_total_variation(const void* inputs, const void* embeddings, void* grad, const int32_t* offsets,
                             float weight, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             uint32_t gridtype, int align_corners, int dtype, ngp_stream_t stream);

/* Diagnostic (no reference counterpart): the per-corner table entry index (before *C) the kernels
 * use, [L,B,2^D] uint32, 0xFFFFFFFF for out-of-range points.  Lets the parity suite check grid
 * indexing bit-for-bit. */
int ngp_grid_corner_indices(const float* inputs, const int32_t* offsets, uint32_t* indices, uint32_t B, uint32_t D,
                            uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                            ngp_stream_t stream);

/* The per-level (scale, resolution) table every grid kernel uses (host computation, no device work):
 * scale_l = fma(exp2((float)l*S), H, -1) in fp32 with a correctly rounded exp2; resolution_l = ceil(scale_l)+1.
 * Restates gridencoder.cu:137-139 with a reproducible exp2. */
int ngp_grid_level_table(uint32_t L, float S, uint32_t H, float* scale_out, uint32_t* resolution_out);

/* Second order (no reference counterpart): the backward of ngp_grid_encode_backward's two outputs with respect to the
 * upstream gradient `u` of grad_inputs (what torch.autograd.grad(..., create_graph=True) on a loss of d enc / d x needs;
 * DESIGN.md "Second order through the grid encoder").  With a_k = sum_d u[b,d] dw_k/dx_d per level, point and corner:
 *   grad_embeddings[i_k,c] += a_k * grad[l,b,c]                      accumulated, pre-zeroed by the caller
 *   grad_grad[l,b,c]        = sum_k a_k * embeddings[i_k,c]           [L,B,C] table dtype, written (NULL: not computed)
 *   grad_inputs2[b,e]       = sum_{l,c} grad[l,b,c] sum_k da_k/dx_e embeddings[i_k,c]   [B,D] table dtype, written (NULL: not computed)
 * grad [L,B,C], grad_grad_inputs (u) [B,D] and the outputs in the table dtype; inputs fp32 in [0,1] (points outside contribute
 * nothing; kinks at cell faces are ignored as in the first backward).  grad_grad and grad_inputs2 are deterministic in every dtype.
 * grad_embeddings: F32 global float atomics; F16 packed fp16 atomics, even C only (odd C: NGP_ERR_INVALID -- autocast only makes
 * fp16 tables for even C); F64 bit-reproducible (record sort, no float atomics), needs a 256-byte aligned workspace of
 * ngp_grid_backward_backward_workspace_bytes(...) bytes and B * 2^D <= 2^31.  NULL grad / inputs / embeddings / offsets /
 * grad_grad_inputs / grad_embeddings: NGP_ERR_INVALID (B == 0 is a no-op).  The v-terms (the backward with respect to the
 * upstream gradient of grad_embeddings) are ngp_grid_encode_forward and the first backward's input term on that table. */
int ngp_grid_encode_backward_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                      const void* grad_grad_inputs, void* grad_grad, void* grad_embeddings, void* grad_inputs2,
                                      uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                      int align_corners, uint32_t interp, int dtype, void* workspace, size_t workspace_bytes,
                                      ngp_stream_t stream);
/* scratch of ngp_grid_encode_backward_backward: 0 for F32 / F16; for F64 a function of B and D alone (offsets_host may be NULL) */
size_t ngp_grid_backward_backward_workspace_bytes(const int32_t* offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, int dtype);

/* Ordered scatter (no reference counterpart): the table gradient of the first and of the second order for F32 and
 * F16 tables WITHOUT float atomics, bit-reproducible.  Every D in {2,3,4,5} and C in {1,2,4,8}, F16 with odd C included (nothing is
 * packed).  Opt-in: the entries above run exactly what they ran.
 * Per level: one record per (point, corner), n = B * 2^D (key = the entry, level_size for a point outside [0,1]^D; value = the slot
 * b << D | k), a stable 8-bit LSD radix sort on bit_length(level_size) bits, then the sum.  THE ORDER OF THE ADDITIONS is part of the
 * contract and a function of the sorted array alone -- not of the launch geometry, the workspace or anything else two calls with equal
 * inputs may differ in: the array is cut into tiles of 64 records; each tile's run of one entry (a fragment) is summed left to right
 * in fp32 starting from its first contribution; a run inside one tile is added once, dst = T(float(dst) + sum); a fragment whose run
 * crosses the tile's left (right) edge becomes the record (entry, partial sum) at slot 2t (2t + 1) of the next array, which is summed
 * by the same rule, until an array fits one tile.  No lane performs more than 63 dependent additions per launch, however the points
 * cluster; the launches and the array sizes follow from (B, D) alone, nothing is read back, the call can be captured in a graph.
 * The contributions come from the atomic paths' code: w_k * grad (first order: the fp32 weight product), a_k * grad (second order: a_k
 * from the fp32 phi, 1 - phi and phi' in double, rounded to fp32 once), one fp32 product each.
 *
 * ngp_grid_encode_backward_ordered: the arguments of ngp_grid_encode_backward_ws without offsets_host; grad_inputs has the bits of
 * ngp_grid_encode_backward.  ngp_grid_encode_backward_backward_ordered: the arguments of ngp_grid_encode_backward_backward;
 * grad_grad and grad_inputs2 have its bits.  grad_embeddings is accumulated (pre-zeroed by the caller).  Both need a 256-byte
 * aligned workspace of ngp_grid_ordered_workspace_bytes(B, D, C, dtype) bytes and B * 2^D <= 2^31; both refuse NGP_F64 (the entries
 * above are bit-reproducible for it).  Everything is checked before any launch; B == 0 is a no-op. */
int ngp_grid_encode_backward_ordered(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                     void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                     const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                     float bound, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
int ngp_grid_encode_backward_backward_ordered(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                              const void* grad_grad_inputs, void* grad_grad, void* grad_embeddings, void* grad_inputs2,
                                              uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                              int align_corners, uint32_t interp, int dtype, void* workspace, size_t workspace_bytes,
                                              ngp_stream_t stream);
/* scratch of the two ordered entries, a function of its arguments alone (0 for B == 0 and for arguments they refuse).  With n = B * 2^D
 * and a256(x) = x rounded up to 256:  4 a256(4 n)  [keys and slots, twice]  +  a256(4 (256 * 1024 + 256))  [radix counts]
 * + sum_i (a256(4 m_i) + a256(4 C m_i))  [partial sums: m_1 = 2 ceil(n / 64), m_{i+1} = 2 ceil(m_i / 64), while m_{i-1} > 64] */
size_t ngp_grid_ordered_workspace_bytes(uint32_t B, uint32_t D, uint32_t C, int dtype);
/* host only: 1 when ngp_grid_encode_backward_ws with these arguments (a workspace and offsets_host given) runs every level without
 * float atomics -- every level on the record-sort path, or NGP_F64 -- else 0 (also for arguments no call accepts) */
int ngp_grid_backward_is_reproducible(const int32_t* offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                      uint32_t gridtype, int align_corners, int dtype);

/* ---------------------------------------------------------------------------------------------
 * shencoder        (reference: shencoder/src/shencoder.h:9-10, bindings.cpp:5-8)
 * --------------------------------------------------------------------------------------------- */

/* replaces sh_encode_forward (shencoder.cu:400-417): inputs [B,3]; outputs [B,C*C]; dy_dx [B,3*C*C] or NULL;
 * D must be 3, C (number of bands) in 1..8.  dtype F32, F16 or F64 (fp64 arithmetic and constants). */
int ngp_sh_encode_forward(const void* inputs, void* outputs, uint32_t B, uint32_t D, uint32_t C, void* dy_dx,
                          int dtype, ngp_stream_t stream);
/* replaces sh_encode_backward (shencoder.cu:419-439): grad_inputs[b,d] += sum_ch grad[b,ch]*dy_dx[b,d,ch] */
int ngp_sh_encode_backward(const void* grad, const void* inputs, uint32_t B, uint32_t D, uint32_t C,
                           const void* dy_dx, void* grad_inputs, int dtype, ngp_stream_t stream);
/* EXTENSION, the backward of sh_encode_backward (shencoder.cu:419-439) for a loss on grad_inputs (torch.autograd.grad(..., create_graph=True)):
 * u [B,3] = d loss / d grad_inputs; grad [B,C*C], inputs [B,3] and dy_dx [B,3*C*C] as the first backward saw them.
 *   grad_grad    [B,C*C]  sum_d u_d dy_dx[b,d,i]                                   (NULL: not computed)
 *   grad_inputs2 [B,3]    sum_i grad_i sum_d u_d d2Y_i/dx_d dx_e                   (NULL: not computed; zeros for C <= 2)
 * Both are overwritten, deterministic, no atomics.  dtype F32 or F64 (F16: NGP_ERR_INVALID, "second order is provided for float32 and
 * float64").  D must be 3, C in 1..8; NULL grad / inputs / dy_dx / u: NGP_ERR_INVALID (B == 0 is a no-op). */
int ngp_sh_encode_backward_backward(const void* grad, const void* inputs, const void* dy_dx, const void* u, uint32_t B, uint32_t D,
                                    uint32_t C, void* grad_grad, void* grad_inputs2, int dtype, ngp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * raymarching      (reference: raymarching/src/raymarching.h:7-18, bindings.cpp:5-19)
 * All floating tensors are fp32 (the reference's wrappers force it with custom_fwd(cast_inputs=float32)).
 * --------------------------------------------------------------------------------------------- */

/* replaces near_far_from_aabb (raymarching.cu:148-156) */
int ngp_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near,
                           float* nears, float* fars, ngp_stream_t stream);
/* replaces sph_from_ray (raymarching.cu:201-209) */
int ngp_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords,
                     ngp_stream_t stream);
/* replaces morton3D / morton3D_invert (raymarching.cu:229-232, 257-260) */
int ngp_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, ngp_stream_t stream);
int ngp_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, ngp_stream_t stream);
/* replaces packbits (raymarching.cu:292-300): N = number of output bytes, grid has 8*N floats */
int ngp_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, ngp_stream_t stream);
/* extension: the threshold is min(density_thresh, *thresh_cap) with thresh_cap a DEVICE scalar (may be NULL) -- the occupancy refresh
 * packs against min(mean_density, density_thresh) (renderer.py:527-529) without reading the mean back to the host */
int ngp_packbits_ex(const float* grid, uint32_t N, float density_thresh, const float* thresh_cap, uint8_t* bitfield,
                    ngp_stream_t stream);

/* replaces march_rays_train (raymarching.cu:482-490).
 * Sample slots are handed out by a deterministic prefix sum in ray order (rays[n] = (n, offset_n,
 * count_n)), which is the allocation a sequential execution of the reference kernel produces;
 * counter[0] += total samples, counter[1] += N.  `workspace` must hold
 * ngp_march_rays_train_workspace_bytes(N) bytes (contents undefined on entry). */
size_t ngp_march_rays_train_workspace_bytes(uint32_t N);
int ngp_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                         uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                         const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays,
                         int32_t* counter, const float* noises, void* workspace, ngp_stream_t stream);

/* replaces composite_rays_train_forward / _backward (raymarching.cu:580-588, 685-693) */
int ngp_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                     float* weights_sum, float* depth, float* image, ngp_stream_t stream);
int ngp_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                      const float* rgbs, const float* deltas, const int32_t* rays,
                                      const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                      float T_thresh, float* grad_sigmas, float* grad_rgbs, ngp_stream_t stream);

/* replaces march_rays / composite_rays (raymarching.cu:808-815, 908-914) */
int ngp_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                   uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars, float* xyzs,
                   float* dirs, float* deltas, const float* noises, ngp_stream_t stream);
int ngp_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive, float* rays_t,
                       const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum,
                       float* depth, float* image, ngp_stream_t stream);

/* fp64 twins of near_far_from_aabb, sph_from_ray, packbits, composite_rays_train_forward / _backward and composite_rays: the same
 * arguments with every floating tensor double (the reference dispatches these on the tensor dtype); the scalars stay float and are
 * widened exactly.  The reference's per-ray loops in fp64 (exp in double, T < T_thresh compared in double); a near/far miss gives
 * DBL_MAX.  (No fp64 marchers.) */
int ngp_near_far_from_aabb_f64(const double* rays_o, const double* rays_d, const double* aabb, uint32_t N, float min_near,
                               double* nears, double* fars, ngp_stream_t stream);
int ngp_sph_from_ray_f64(const double* rays_o, const double* rays_d, float radius, uint32_t N, double* coords, ngp_stream_t stream);
int ngp_packbits_f64(const double* grid, uint32_t N, float density_thresh, uint8_t* bitfield, ngp_stream_t stream);
int ngp_composite_rays_train_forward_f64(const double* sigmas, const double* rgbs, const double* deltas, const int32_t* rays,
                                         uint32_t M, uint32_t N, float T_thresh, double* weights_sum, double* depth, double* image,
                                         ngp_stream_t stream);
int ngp_composite_rays_train_backward_f64(const double* grad_weights_sum, const double* grad_image, const double* sigmas,
                                          const double* rgbs, const double* deltas, const int32_t* rays, const double* weights_sum,
                                          const double* image, uint32_t M, uint32_t N, float T_thresh, double* grad_sigmas,
                                          double* grad_rgbs, ngp_stream_t stream);
int ngp_composite_rays_f64(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive, double* rays_t,
                           const double* sigmas, const double* rgbs, const double* deltas, double* weights_sum, double* depth,
                           double* image, ngp_stream_t stream);

/* Extension (no reference counterpart): stream compaction of the alive list on the
 * device, replacing `rays_alive[rays_alive >= 0]` + its host sync in the caller's render loop.
 * out_alive receives the surviving ids in order, *out_count (device int32) their number. */
size_t ngp_compact_rays_workspace_bytes(uint32_t n_alive);
int ngp_compact_rays(const int32_t* rays_alive, uint32_t n_alive, int32_t* out_alive, int32_t* out_count,
                     void* workspace, ngp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ffmlp            (reference: ffmlp/src/ffmlp.h:8-14, bindings.cpp:5-11)
 * All tensors fp16.  weights: flat [hidden*in] + (num_layers-1) x [hidden*hidden] + [output_dim*hidden],
 * each matrix row-major [out,in].  B must be a multiple of 128 (the wrapper pads), hidden_dim in
 * {16,32,64,128,256}, input_dim % 16 == 0, output_dim == 16 (padded by the wrapper), num_layers >= 2 -- the reference's own
 * constraints (ffmlp.py:112-115, ffmlp.cu:543-556,653-658).  Register-resident kernels serve hidden_dim <= 128 forward and the
 * instant-ngp shapes backward (hidden 32/64, <= 4 hidden layers, input_dim <= 64); every other shape runs the layered kernels
 * (one matmul's weights in LDS at a time).  The only shapes refused (NGP_ERR_INVALID) are those whose single largest
 * layer exceeds the LDS: hidden_dim * max(input_dim, hidden_dim) * 2 bytes > 152 KiB, i.e. input_dim > 304 with 256-wide layers.
 * activation ids: 0 ReLU, 1 Exp, 2 Sine, 3 Sigmoid, 4 Squareplus, 5 Softplus, 6 None (utils.h:29-37).
 * `activation` is the hidden layers' one, `output_activation` is applied to the output matmul and is FORWARD-ONLY: the backward ignores it
 * (grad is taken as the gradient of what the output matmul produced, as in the reference, ffmlp.cu:780).  The backward takes the derivative
 * from the STORED post-activations y (ReLU y > 0, Exp y, Sigmoid y(1-y), Squareplus s^2/(s^2+1) with s = 10y, Softplus 1 - exp(-10y),
 * None 1: utils.h:532-582); Sine back-propagates as the identity -- cos(x) cannot be recovered from sin(x), the reference passes it through too.
 * --------------------------------------------------------------------------------------------- */

/* replaces ffmlp_forward (ffmlp.cu:635-671): forward_buffer [num_layers,B,hidden] receives the hidden
 * post-activations in a layout private to this library (only ngp_ffmlp_backward reads it). */
int ngp_ffmlp_forward(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                      uint32_t hidden_dim, uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                      void* forward_buffer, void* outputs, ngp_stream_t stream);
/* replaces ffmlp_inference (ffmlp.cu:673-709): inference_buffer [B,hidden] is scratch (used by the layered kernel only) */
int ngp_ffmlp_inference(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                        uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                        uint32_t output_activation, void* inference_buffer, void* outputs, ngp_stream_t stream);
/* replaces ffmlp_backward (ffmlp.cu:749-895): grad [B,output_dim]; backward_buffer [num_layers,B,hidden]
 * scratch; grad_inputs [B,input_dim] written iff calc_grad_inputs; grad_weights flat fp16: OVERWRITTEN with the
 * fp32-accumulated batch sums rounded once to fp16 whatever it held (the reference's wrapper zero-fills it,
 * ffmlp.py:66-71: not needed here) -- also for an empty batch (B == 0: zeros). */
int ngp_ffmlp_backward(const void* grad, const void* inputs, const void* weights, const void* forward_buffer,
                       uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                       uint32_t activation, uint32_t output_activation, int calc_grad_inputs, void* backward_buffer,
                       void* grad_inputs, void* grad_weights, ngp_stream_t stream);
/* replace allocate_splitk / free_splitk (ffmlp.cu:721-740).  The reference creates size streams+events
 * for its split-K weight-gradient GEMMs; this library reduces weight gradients inside the backward
 * kernel, so these only record the request (kept so that FFMLP.__init__ runs unchanged). */
int ngp_allocate_splitk(size_t size);
int ngp_free_splitk(void);

/* ---------------------------------------------------------------------------------------------
 * Fused sample pipeline -- EXTENSIONS beyond the reference surface.
 * The reference wrappers glue the native ops with permute/cat/cast/elementwise PyTorch kernels
 * (grid.py:57,75,149; ffmlp.py:157-165; network_ff.py:51-123).  These entry points let the mirror in
 * torch-ngp_amd/ run the same arithmetic with the same rounding points and no glue copies; the
 * reference-contract functions above are thin wrappers over them (flags = 0, bound = 0).
 * --------------------------------------------------------------------------------------------- */
/* bound > 0: inputs are world coordinates in [-bound, bound], mapped in-kernel as (x + bound) * (1/(2 bound))
 * (what GridEncoder.forward does with two PyTorch kernels, grid.py:149); bound == 0: unit inputs. */
int ngp_grid_encode_forward_ex(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                               uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                               uint32_t gridtype, int align_corners, uint32_t interp, int dtype, float bound,
                               ngp_stream_t stream);
int ngp_grid_encode_backward_ex(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners,
                                uint32_t interp, int dtype, float bound, ngp_stream_t stream);
/* grid_encode_forward_ex with relative per-level costs from the caller (HOST array of L positive floats, e.g. the expected fraction of
 * consecutive samples that change cell at each level): the launch's per-XCD work lists are balanced by them -- whole levels stay on XCD
 * (level mod 8), the tail of the most loaded XCDs' last level moves to the least loaded ones.  Scheduling only: the arithmetic per
 * (level, point) and the results are identical.  level_cost_host == NULL: ngp_grid_encode_forward_ex (every level costs the same). */
int ngp_grid_encode_forward_sched(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                                  uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                                  uint32_t gridtype, int align_corners, uint32_t interp, int dtype, float bound,
                                  const float* level_cost_host, ngp_stream_t stream);

/* ngp_grid_encode_forward_sched for a DOUBLE-BUFFERED fp16 table (ngp_table_adam_t): the kernel reads *parity (a device float: the
 * optimizer's state[5]) at entry and gathers from `embeddings` when it is 0, from `embeddings_alt` otherwise -- the selection is made on the
 * device, so a captured HIP graph follows the commit / skip decisions of the steps replayed before it.  embeddings_alt == NULL or parity ==
 * NULL: ngp_grid_encode_forward_sched.  dy_dx must be NULL (the inference / fused-training forward).
 * rows_dev (optional device word, independent of the table selection): only the first min(B, *rows_dev) points are encoded -- the launch is sized
 * for B, workgroups behind the device-side count leave at once (the eval loop's emitted-row count, ngp_march_rays_dev_rows). */
int ngp_grid_encode_forward_sel(const float* inputs, const void* embeddings, const void* embeddings_alt, const float* parity,
                                const uint32_t* rows_dev, const int32_t* offsets, void* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype, float bound,
                                const float* level_cost_host, ngp_stream_t stream);

/* diagnostic: the per-XCD work lists ngp_grid_encode_forward_sched would launch for L levels of `tiles` tiles each (host computation):
 * 8 x 8 segments (level, first tile, cumulative slot end; level 0xffff = unused); returns the slots of the longest list (0 on bad arguments) */
uint32_t ngp_grid_forward_work_lists(uint32_t L, uint32_t tiles, const float* level_cost_host, uint16_t* level_out, uint32_t* tile0_out,
                                     uint32_t* end_out);

/* grid_encode_backward_ex with a caller-provided workspace: fp16 tables with C = 2 and D <= 3 (the instant-ngp configuration) then
 * run EVERY level WITHOUT memory-side atomics -- contributions are sorted by table slice (12-byte pair units = 6 bytes per record,
 * coalesced stores) and each slice is summed exactly in a 64-bit fixed-point LDS accumulator, rounded once and added to grad_embeddings
 * by the workgroup that owns it.  The result is the exact sum of the fp16 contributions rounded once (the reference's atomics round after every
 * add, in an undefined order) and is bit-reproducible; entries that receive a non-finite contribution become NaN.
 * offsets_host: a HOST copy of `offsets` (L + 1 values; the level sizes steer the plan).  workspace: device memory of at least
 * ngp_grid_backward_workspace_bytes(...) bytes, contents irrelevant.  offsets_host == NULL or workspace == NULL -> the atomic path
 * (= ngp_grid_encode_backward_ex).  Small batches and other dtypes/shapes use the atomic path as well (workspace_bytes() == 0).
 * NGP_F64 (this entry and _ws only; the _checked entries refuse it): the backward is bit-reproducible -- per level, one record per
 * (point, corner) contribution, a stable radix sort on the table entry, each entry's contributions summed in fp64 in point order and
 * added once (no float atomics).  Its workspace is a function of B and D alone (offsets_host may be NULL, e.g. during stream capture):
 * ngp_grid_backward_workspace_bytes(NULL, B, D, ..., NGP_F64) bytes, 256-byte aligned, required; B * 2^D <= 2^31. */
size_t ngp_grid_backward_workspace_bytes(const int32_t* offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                         uint32_t gridtype, int align_corners, int dtype);
/* ngp_grid_encode_backward_ws that also does the optimizer's non-finite sweep over the gradient table where the values are produced:
 * found_inf (optional device float) is set to 1 when a gradient entry this call wrote is not finite (needs offsets_host; levels that
 * went through atomics are swept by one extra launch).  With it, ngp_optim_adam_step_ex can be called without its CHECK phase. */
int ngp_grid_encode_backward_checked(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                     void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                     const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp,
                                     int dtype, float bound, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
                                     float* found_inf, ngp_stream_t stream);

/* ngp_grid_encode_backward_checked that also CARRIES the deferred slab reduction of two FFMLP backward launches (NGP_FF_DEFER_REDUCE; same
 * arguments and results as ngp_ffmlp_reduce_slabs_pair, found_inf shared) in its own last launch instead of a launch of ~270 small blocks
 * behind it: the two are independent, the reduction fills slots the last table slices leave idle (training step: -1 launch, ~6 us).
 * slab_sets == NULL: plain ngp_grid_encode_backward_checked.  When this call has no such launch (few samples, no workspace, B == 0) the
 * reduction is launched on its own: the reduced gradients are there when the call returns either way (stream order). */
/* Adam on the hash table INSIDE the slice accumulate of the grid backward (round 6).  torch.optim.Adam + GradScaler.step
 * (nerf/utils.py:751-753) need the global "any gradient non-finite?" verdict before the first weight moves; the accumulate produces the final
 * gradient of a 4096-entry slice in LDS while most of the chip waits on its record walk, and a separate 28 B/parameter Adam sweep over the
 * 12 M-entry table follows.  Here the flush of every slice applies Adam at once -- SPECULATIVELY: it reads the parameters, moments of buffer
 * set state[5] (the parity: 0 or 1) and writes the updated parameters, moments and fp16 shadow into the OTHER set.  The commit
 * (ngp_optim_adam_small_commit / NGP_OPT_PHASE_FLIP) flips the parity only when the step stands; a skipped step leaves the current set
 * untouched -- GradScaler's semantics, exactly.  Readers of the fp16 table select the current set at kernel entry
 * (ngp_grid_encode_forward_sel).  Needs overwrite_table with every level on the record-sort path (else NGP_ERR_INVALID: nothing was
 * launched); the fp16 gradient is rounded exactly as when it is stored, so the result equals ngp_optim_adam_step_ex on the stored gradient
 * bit for bit.  The DENSE levels at the start of the table (their entries are dealt round-robin to the accumulate's workgroups: 8-byte
 * accesses 1 KiB apart would be all the flush could do for them) are left out: their gradient is stored to grad_embeddings as usual and
 * ngp_optim_adam_small_commit sweeps that prefix contiguously (same double buffer, verdict already known) -- ngp_grid_table_adam_prefix()
 * entries.  Behind the prefix grad_embeddings is not written (it may be NULL when the prefix is empty). */
typedef struct ngp_table_adam {
    float* param[2]; float* exp_avg[2]; float* exp_avg_sq[2]; void* param_fp16[2];   /* [n_entries, C] each; set index = parity */
    const float* state;          /* the optimizer's scalars (ngp_optim_adam_step: state[0] scale, [3] step count, [4] lr multiplier, [5] parity) */
    float lr, beta1, beta2, eps;
} ngp_table_adam_t;
/* entries (whole levels) at the start of the table that a backward with table_adam leaves to ngp_optim_adam_small_commit; 0xffffffff: this
 * batch / table shape cannot carry the sweep at all (the backward would refuse table_adam).  Host computation, same plan as the backward. */
uint32_t ngp_grid_table_adam_prefix(const int32_t* offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                    uint32_t gridtype, int align_corners, int dtype);
typedef struct ngp_slab_sets {
    const void* slabs_a; uint32_t n_slabs_a, n_params_a; void* grad_weights_a;
    const void* slabs_b; uint32_t n_slabs_b, n_params_b; void* grad_weights_b;
    /* optional third carried job: loss[0] = sum(ray_err[0 .. n_rays)) / (3 n_rays), the loss VALUE ngp_composite_train_loss_backward would
     * have summed itself (call it with loss = NULL: its workgroups then skip the ticket round trip); same routine, same bits.  loss = NULL: none */
    const float* ray_err; uint32_t n_rays; float* loss;
    /* != 0: grad_embeddings receives this call's gradient instead of having it ADDED (every entry is written, zeros included, nothing is
     * read): for a caller whose optimizer then does not zero the buffer (ngp_optim_adam_step*: grad_is_half & 2).  Same bits as adding into
     * a zeroed buffer.  Calls that cannot write every entry from the sort (levels on the atomic path) zero the table first. */
    uint32_t overwrite_table;
    /* optional (NULL: none): the table's Adam sweep rides in the accumulate's flush, see ngp_table_adam_t */
    const ngp_table_adam_t* table_adam;
} ngp_slab_sets_t;
int ngp_grid_encode_backward_checked_slabs(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                           void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                           const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp,
                                           int dtype, float bound, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
                                           float* found_inf, const ngp_slab_sets_t* slab_sets, ngp_stream_t stream);
int ngp_grid_encode_backward_ws(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp,
                                int dtype, float bound, const int32_t* offsets_host, void* workspace, size_t workspace_bytes,
                                ngp_stream_t stream);

/* The apply half of the occupancy-grid refresh (NeRFRenderer.update_extra_state, nerf/renderer.py:515-529) in three launches instead of
 * ~15 PyTorch ones: `tmp_grid[cas, indices] = sigmas` (scatter of density_scale * sigmas), the EMA-max update
 * `grid = max(grid * decay, tmp)` where both sides are >= 0 (one update per distinct cell), `mean(clamp(grid, 0))` (double, fixed order)
 * and packbits against min(density_thresh, mean) -- nothing read back.  cells [n] int64: cascade * H^3 + morton index of each queried
 * point; scratch [n_cells] fp32: -1 everywhere before the first call, left that way; workspace: ngp_density_grid_update_workspace_bytes,
 * zeroed before the first call.
 * What tests/test_gpu_occupancy.py pins (model: tests/occupancy_cases.py density_update_model):
 *   - n_cells >= 8 and a multiple of 8; density_grid and scratch 16-byte aligned (NGP_ERR_INVALID otherwise); n may be 0;
 *   - an index >= n_cells is ignored (nothing is written for it); indices are not expected to be negative;
 *   - with f = fl32(density_scale * sigma) the fresh value of a sampled cell and g its grid value: where g >= 0 and f >= 0 (-0.0 counts
 *     as >= 0) the cell becomes max(fl32(g * decay), f) in fp32 (max(+0, -0) = +0), bit for bit; a NaN or negative f is NOT applied -- its
 *     scratch entry is reset to -1 all the same --, a cell with g < 0 is left alone, a cell that was not sampled keeps its bits (no
 *     decay).  Of several samples of one cell any one wins (as with index_put_);
 *   - scratch is -1.0 everywhere after every call, the workspace is ready for the next call (no re-zeroing);
 *   - mean_out[0] = the fp32 rounding of [sum of max(g, 0) over the updated grid, accumulated in double in a fixed order] / n_cells: the
 *     same bits on every call with the same inputs, at most 1 fp32 ulp from the rounding of the exact mean (equal to it when the double
 *     sum is exact in any order);
 *   - bitfield = packbits(updated grid, fminf(density_thresh, mean_out[0])). */
size_t ngp_density_grid_update_workspace_bytes(uint32_t n_cells);
int ngp_density_grid_update(const float* sigmas, const int64_t* cells, uint32_t n, float density_scale, float decay, float* density_grid,
                            uint32_t n_cells, float* scratch, float density_thresh, float* mean_out, uint8_t* bitfield, void* workspace,
                            ngp_stream_t stream);

/* flags of the ffmlp *_ex entry points */
#define NGP_FF_INPUT_PLANAR 1u /* inputs are [input_dim/2][B][2] fp16 planes = the grid encoder's [L,B,C=2] output */
#define NGP_FF_DX_PLANAR 2u    /* grad_inputs is written in that planar layout = what grid_encode_backward reads */
#define NGP_FF_LAYERED 4u      /* testing: force the layered kernels on shapes the register-resident ones would serve */
#define NGP_FF_SINGLE_WAVE 8u  /* testing: backward with one wave per tile stream instead of the paired kernel (2- and 3-layer nets) */
#define NGP_FF_DEFER_REDUCE 16u /* backward of a 2- / 3-layer net: leave the per-workgroup fp32 weight-gradient slabs in backward_buffer; the
                                 * caller sums them later (ngp_ffmlp_reduce_slabs_pair), e.g. two networks' slabs in one launch */
#define NGP_FF_RECOMPUTE 32u   /* backward of a 64-wide ReLU net with 32 inputs and 2 / 3 layers: forward_buffer is not read (may be NULL); the
                                 * hidden activations are recomputed from `inputs` -- bit for bit what the forward pass would have stored.
                                 * ngp_network_forward(training) with both forward buffers NULL is the matching forward: it does not store them */
#define NGP_FF_SERIAL_FLUSH 64u /* testing: the register-resident backward kernels sum their waves' weight-gradient accumulators in the reference
                                 * form -- one wave after the other into one LDS copy -- instead of the staged parallel sum; same additions in
                                 * the same order, so the same bits (tests/test_gpu_ffmlp_slab_sum.py).  No effect on the shapes that only have the
                                 * serial form: the layered kernels, the paired kernel of 64-wide 3-layer nets with more than 32 inputs, the
                                 * single-wave kernel of 64-wide nets with 3 or 4 layers */
int ngp_ffmlp_forward_ex(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                         uint32_t hidden_dim, uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                         void* forward_buffer, void* outputs, uint32_t flags, ngp_stream_t stream);
int ngp_ffmlp_inference_ex(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                           uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                           uint32_t output_activation, void* inference_buffer, void* outputs, uint32_t flags,
                           ngp_stream_t stream);
int ngp_ffmlp_backward_ex(const void* grad, const void* inputs, const void* weights, const void* forward_buffer,
                          uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                          uint32_t activation, uint32_t output_activation, int calc_grad_inputs, void* backward_buffer,
                          void* grad_inputs, void* grad_weights, uint32_t flags, ngp_stream_t stream);

/* ffmlp_backward with a caller-provided workspace (ngp_ffmlp_backward_workspace_bytes(...) bytes; 0 for the shapes served by the
 * register-resident kernels): the layered path splits the batch reduction of the weight gradients over sample chunks and keeps one fp32
 * slab per chunk there.  workspace == NULL: one chunk (same results to fp32 summation order, less parallelism). */
size_t ngp_ffmlp_backward_workspace_bytes(uint32_t B, uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers);
int ngp_ffmlp_backward_ws(const void* grad, const void* inputs, const void* weights, const void* forward_buffer, uint32_t B,
                          uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                          uint32_t output_activation, int calc_grad_inputs, void* backward_buffer, void* grad_inputs, void* grad_weights,
                          uint32_t flags, void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* Second order (no reference counterpart): the backward of ngp_ffmlp_backward's outputs with respect to the upstream gradient `u`
 * [B,input_dim] of grad_inputs -- what torch.autograd.grad(..., create_graph=True) on a loss of d y / d x (eikonal, normals) needs;
 * DESIGN.md 3.7 has the formulas.  grad [B,16], inputs [B,input_dim], weights, u: fp16 row-major; forward_buffer as ngp_ffmlp_forward*
 * left it (private layout).  Outputs, all fp16, all written (not accumulated), each nullable -- a NULL output skips the terms that
 * feed only it:
 *   grad_grad     [B,16]        d loss / d grad
 *   grad_weights2 [n_params]    d loss / d weights, the layout of `weights`; bit-reproducible (fp32 slabs, one fixed-order reduction)
 *   grad_inputs2  [B,input_dim] d loss / d inputs; exactly zero for ReLU, Sine and None (written as zeros)
 * The terms with respect to the upstream gradient of grad_weights are not provided.  Every width runs the layered kernels; the
 * workspace (ngp_ffmlp_backward_backward_workspace_bytes(...) bytes, 256-byte aligned) holds the recomputed hidden gradients, the
 * tangents and the weight-gradient slabs.  B a multiple of 128 (0: no-op), output_dim 16.  A bad shape, a NULL grad / inputs /
 * weights / forward_buffer / u or a short workspace: NGP_ERR_INVALID before anything is launched. */
size_t ngp_ffmlp_backward_backward_workspace_bytes(uint32_t B, uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers,
                                                   uint32_t activation);
int ngp_ffmlp_backward_backward(const void* grad, const void* inputs, const void* weights, const void* forward_buffer, const void* u,
                                uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                                uint32_t activation, void* grad_grad, void* grad_weights2, void* grad_inputs2, void* workspace,
                                size_t workspace_bytes, ngp_stream_t stream);

/* The whole network of nerf/network_ff.py:51-74 behind the encoder in ONE launch (64-wide ReLU networks with 32 inputs, the instant-ngp
 * configuration): sigma FFMLP -> trunc_exp / SH(4) / feature shuffle -> colour FFMLP -> sigmoid.  enc: the encoder output, [M,32] fp16
 * row-major or (flags & NGP_FF_INPUT_PLANAR) the encoder's own [16][M][2] layout; dirs [M_valid,3] fp32 (rows >= M_valid use dir = 0);
 * -> sigma [M] fp32 (= density_scale * exp(h0)), rgb [M,3] fp32.  training != 0 also writes what ngp_ffmlp_backward* and the
 * ngp_pipeline_*_backward kernels read: forward_buffer_sigma [nl_s,M,64], h16 [M,16], color_in [M,32], forward_buffer_color [nl_c,M,64]
 * (all fp16, the forward buffers in this library's private layout; both forward buffers NULL: not stored, for a backward that runs with
 * NGP_FF_RECOMPUTE).  Bit-identical to the sequence ngp_ffmlp_forward_ex ->
 * ngp_pipeline_mid_forward -> ngp_ffmlp_forward_ex -> ngp_pipeline_rgb_forward it replaces. */
int ngp_network_forward(const void* enc, const float* dirs, uint32_t M, uint32_t M_valid, const void* w_sigma, const void* w_color,
                        uint32_t num_layers_sigma, uint32_t num_layers_color, float density_scale, int training,
                        void* forward_buffer_sigma, void* h16, float* sigma, void* color_in, void* forward_buffer_color, float* rgb,
                        uint32_t flags, ngp_stream_t stream);

/* ngp_network_forward whose launch is sized for M rows but evaluates only the first ceil(*rows_dev / 32) tiles (rows_dev: optional device word, the
 * eval loop's emitted-row count; NULL: ngp_network_forward).  Buffer strides follow M. */
int ngp_network_forward_rows(const void* enc, const float* dirs, uint32_t M, uint32_t M_valid, const void* w_sigma, const void* w_color,
                             uint32_t num_layers_sigma, uint32_t num_layers_color, float density_scale, int training,
                             void* forward_buffer_sigma, void* h16, float* sigma, void* color_in, void* forward_buffer_color, float* rgb,
                             uint32_t flags, const uint32_t* rows_dev, ngp_stream_t stream);

/* Extensions for the fused training iteration (the backward of network_ff.py:40-74):
 *  - ngp_network_backward_color = ngp_ffmlp_backward_ex of the colour MLP (32 -> 64 x (n-1) -> 16, ReLU, n = 2 or 3) whose input-gradient
 *    epilogue writes the sigma net's output gradient grad_h16 [M,16] directly (what ngp_pipeline_mid_backward would assemble from
 *    grad_sigma [M], h16 [M,16] and dL/d(colour input)[:,16:31]); same bits, one launch and a [M,32] round trip less.
 *    flags: 0, NGP_FF_DEFER_REDUCE, NGP_FF_RECOMPUTE (forward_buffer_color may then be NULL), NGP_FF_SERIAL_FLUSH.
 *  - ngp_ffmlp_backward_slab_count: how many fp32 slabs [n_params] a deferred backward of that shape leaves at the start of its
 *    backward_buffer (0: the gradients were stored directly, nothing to sum).
 *  - ngp_ffmlp_reduce_slabs_pair: sums two slab sets (n_slabs x n_params fp32 each, either may be empty) into fp16 weight
 *    gradients in ONE launch, in the fixed order of the single-set reduction (deterministic, same bits).  found_inf (optional device
 *    float): set to 1 when a resulting gradient is not finite -- the optimizer's non-finite sweep (ngp_optim_adam_step_ex, phase
 *    CHECK) done by the producer; a set with n_slabs = 0 (gradients already stored) is then only swept. */
int ngp_network_backward_color(const void* grad_out16, const void* color_in, const void* w_color, const void* forward_buffer_color, uint32_t M,
                               uint32_t num_layers_color, void* backward_buffer, const float* grad_sigma, const void* h16,
                               float density_scale, void* grad_h16, void* grad_w_color, uint32_t flags, ngp_stream_t stream);
uint32_t ngp_ffmlp_backward_slab_count(uint32_t B, uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers);
int ngp_ffmlp_reduce_slabs_pair(const void* slabs_a, uint32_t n_slabs_a, uint32_t n_params_a, void* grad_weights_a, const void* slabs_b,
                                uint32_t n_slabs_b, uint32_t n_params_b, void* grad_weights_b, float* found_inf, ngp_stream_t stream);

/* The row bound of the training chain (additive: the ABI version stays).  The training march publishes a device word -- word 0 of its
 * workspace (ngp_march_rays_train_workspace_bytes), the end of the written row prefix -- and the per-sample kernels behind it, launched for
 * the M rows of their buffers, then work on the rows [0, live) only:
 *     live = min(M, *rows_dev rounded up to a multiple of 512)
 * (512 = the record sort's chunk, a multiple of the MLP tile; ONE rule, csrc/common.h live_rows).  M stays the stride of every buffer and of
 * the workspaces; output rows >= live are NOT written, input rows >= live are not read.  The rows [*rows_dev, live) must be defined: the
 * march zeroes their positions, directions and deltas, the fused compositor their gradients (a zero gradient times an undefined activation
 * would be NaN).  The word is read on the device when a kernel runs: a captured graph or a command list follows the march of the step it
 * replays.
 * ngp_training_row_bound(rows_dev) ARMS the bound on the calling thread; it stays armed until ngp_training_row_bound(NULL).  The signatures
 * of the entries stay what they are (callers, and tools that wrap an entry by its name, see the same calls).  While it is armed, calls on
 * that thread of
 *   ngp_grid_encode_forward_sched / _sel  (fp16 / fp32, no dy_dx; _sel's own rows_dev -- an EXACT count, the eval march publishes it padded --
 *                                         wins when given)
 *   ngp_network_forward / _rows           (likewise: its own rows_dev wins)
 *   ngp_network_backward_color
 *   ngp_ffmlp_backward_ex                 (served by the paired kernel: register-resident 2- / 3-layer nets without NGP_FF_SINGLE_WAVE /
 *                                         NGP_FF_LAYERED; refused otherwise -- NGP_ERR_INVALID, nothing launched.  A workgroup without live
 *                                         tiles still leaves its all-zero slab: the slab count follows M)
 *   ngp_grid_encode_backward_checked_slabs (record sort, slice accumulate -- the flush of every slice, the table's Adam sweep and the carried
 *                                         reductions run whatever the bound, 0 included -- and the atomic levels; refused with dy_dx /
 *                                         grad_inputs)
 * take it; every other entry, and every call while nothing is armed, is unchanged. */
int ngp_training_row_bound(const uint32_t* rows_dev);

/* network_ff.py:55-72 between the two MLPs: h16 [M,16] fp16 (sigma-net output), dirs [M_valid,3] fp32 ->
 * sigma [M] fp32 = exp(h[:,0]) (trunc_exp), color_in [M,32] fp16 = [SH deg 4 | h[:,1:16] | 0]; rows >= M_valid use dir = 0 */
int ngp_pipeline_mid_forward(const void* h16, const float* dirs, float* sigma, void* color_in, uint32_t M, uint32_t M_valid,
                             float density_scale, ngp_stream_t stream);
/* rgb [M,3] fp32 = fp16-rounded sigmoid of the colour net's first three outputs (network_ff.py:72) */
int ngp_pipeline_rgb_forward(const void* out16, float* rgb, uint32_t M, ngp_stream_t stream);
/* grad_out16 [M,16] fp16: columns 0..2 = grad_rgb * y (1 - y), the rest 0 */
int ngp_pipeline_rgb_backward(const float* grad_rgb, const float* rgb, void* grad_out16, uint32_t M, ngp_stream_t stream);
/* grad_h16 [M,16] fp16: column 0 = grad_sigma * exp(clamp(h0, -15, 15)) (activation.py:12-17), columns 1..15 =
 * grad_color_in[:,16:31].  A NaN h0 gives a NaN in column 0 (torch's clamp propagates it), here and in the epilogue of
 * ngp_network_backward_color: the optimizer's non-finite sweep then sees it. */
int ngp_pipeline_mid_backward(const float* grad_sigma, const void* h16, const void* grad_color_in, void* grad_h16, uint32_t M,
                              float density_scale, ngp_stream_t stream);

/* The Trainer's loss (nerf/utils.py:516,557: MSELoss(reduction='none')(pred, gt).mean(-1).mean()) and its gradient times the loss scale
 * in one launch: loss[0] = mean((image - target)^2) over n values, grad_image[i] = (2/n * (image[i] - target[i])) * loss_scale[0]
 * (loss_scale: device scalar, NULL = 1).  Deterministic (fixed-order reduction).  n must be > 0. */
int ngp_pipeline_mse_loss(const float* image, const float* target, uint32_t n, const float* loss_scale, float* loss,
                          float* grad_image, ngp_stream_t stream);

/* nn.Linear stack <-> the flat fp16 weight vector of the fused MLP (the reference's non---ff model, nerf/network.py:32-63 + 155-215, runs its
 * bias-free Linear / ReLU stacks on the ffmlp kernels: torch-ngp_amd/nerf/network.py).  weights[l]: fp32 [out_l, in_l] row major, layer 0
 * [hidden, n_in], layers 1 .. depth-2 [hidden, hidden], layer depth-1 [n_out, hidden] (n_out <= 16).  flat (ngp_linear_stack_flat_size
 * elements): half(W_0) with its columns zero-padded to a multiple of 16 | an exact identity [hidden, hidden] when `identity` (a stack with ONE
 * hidden layer: the kernels want two) | half(W_1 .. W_{depth-2}) | half(W_{depth-1}) zero-padded to 16 rows -- the layout of
 * ngp_ffmlp_forward's `weights`.  unpack_grad: the flat fp16 weight gradient back into fp32 tensors of the layers' shapes (every element
 * written; the padding's and the identity's gradient are dropped).  One launch each (PyTorch's pad / eye / cat and their autograd: ~8). */
#define NGP_LINEAR_STACK_MAX 8
uint32_t ngp_linear_stack_flat_size(uint32_t depth, uint32_t n_in, uint32_t hidden, uint32_t n_out, int identity);
int ngp_linear_stack_pack(const float* const* weights, uint32_t depth, uint32_t n_in, uint32_t hidden, uint32_t n_out, int identity,
                          void* flat_fp16, ngp_stream_t stream);
int ngp_linear_stack_unpack_grad(const void* grad_flat_fp16, uint32_t depth, uint32_t n_in, uint32_t hidden, uint32_t n_out, int identity,
                                 float* const* grads, ngp_stream_t stream);

/* dst [dst_rows, dst_cols] fp16 = src [src_rows, src_cols] (rows src_row_stride elements apart) in its top-left corner, zeros elsewhere: the row /
 * column padding ngp_ffmlp_forward wants (rows to a multiple of 128, columns to 16), one launch. */
int ngp_pad_2d_fp16(const void* src, uint32_t src_rows, uint32_t src_cols, uint32_t src_row_stride, void* dst, uint32_t dst_rows,
                    uint32_t dst_cols, ngp_stream_t stream);

/* Data path: the arithmetic of get_rays (nerf/utils.py:53-137).  poses [B,4,4] row-major camera-to-world; pixel
 * indices inds [B,N] int64 (inds_batch_stride = N) or [N] shared by every pose (inds_batch_stride = 0) or NULL (pixel n = n: a full
 * H x W frame with N = H * W); pixel p is (column p % W, row p / W), sampled at its centre.  rays_o, rays_d [B,N,3] fp32:
 * rays_d = normalize(((col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy, 1)) . R^T,  rays_o = camera position. */
int ngp_rays_from_pixels(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t W, const int64_t* inds,
                         uint32_t inds_batch_stride, uint32_t N, float* rays_o, float* rays_d, ngp_stream_t stream);

/* march_rays_train with two conveniences for the fused renderer: the counter may be reset in-kernel and the sample rows no ray
 * writes are zeroed in-kernel (the reference contract keeps both with the caller: counter.zero_(), torch.zeros buffers). */
#define NGP_MARCH_RESET_COUNTER 1u
#define NGP_MARCH_ZERO_TAIL 2u
#define NGP_MARCH_SCAN_LAUNCH 8u /* testing: keep the separate scan launch between the passes (default with NGP_MARCH_RESET_COUNTER and
                                  * N <= 8192 rays: the write pass hands out the sample slots itself -- same slots, one launch less) */
#define NGP_MARCH_NOISE_FROM_SEED 4u /* `noises` points to ONE device uint32 (a seed that the caller changes from step to step) instead of N
                                      * floats: ray n starts at near + dt * u(n, seed), u a counter-based uniform draw in [0, 1) */
int ngp_march_rays_train_ex(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                            uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                            const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                            const float* noises, void* workspace, uint32_t flags, ngp_stream_t stream);
/* the same with near_far_from_aabb (raymarching.cu:92-145) folded into the first pass: nears / fars [N] are OUTPUTS, computed from the
 * box aabb [6] and min_near with that function's arithmetic (one launch less per training iteration) */
int ngp_march_rays_train_aabb(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                              uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* aabb, float min_near,
                              float* nears, float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                              const float* noises, void* workspace, uint32_t flags, ngp_stream_t stream);

/* march_rays (inference) that zeroes every sample slot it does not fill: the unused tail of each ray's n_step slots and the rows
 * between n_alive*n_step and zero_rows (>= n_alive*n_step), so the buffers need no memset; noises may be NULL (= no perturbation). */
int ngp_march_rays_ex(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t, const float* rays_o,
                      const float* rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                      const uint8_t* grid, const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                      const float* noises, uint32_t zero_rows, ngp_stream_t stream);

/* On-device inference loop: march_rays / composite_rays / alive-list compaction of NeRFRenderer.run_cuda's eval
 * branch (renderer.py:322-367) with the loop state on the DEVICE: state = int32[2] {n_alive, samples marched per ray so far}.  The host
 * launches for an upper bound `alive_bound` of the alive count (the value it last read back) and may issue many iterations between
 * read-backs; the kernels take the true count from `state`, derive n_step = max(min(n_total / n_alive, cap), 1) from it (renderer.py:349:
 * cap = 8 = n_step_cap 0; a caller may raise the cap for the tail of a frame, where a handful of surviving rays would otherwise need one
 * launch set per 8 samples -- a ray's samples and their compositing order do not depend on the chunking, the SAME n_total and n_step_cap
 * must go to the three calls of one iteration), and do nothing for lanes beyond it.  march: sample rows [n_alive * n_step, rows) are
 * zero-filled (rows >= min(n_total, cap * alive_bound) always suffices); noises may be NULL.  compact: writes the surviving ids in order to out_alive and the next iteration's state to
 * out_state (count forced to 0 once max_steps samples were marched); workspace: ngp_compact_rays_workspace_bytes(alive_bound).
 * Slot layout, n_step sequence and compaction order equal the host-driven loop's, so do the results. */
int ngp_march_rays_dev(const int32_t* state, uint32_t alive_bound, uint32_t n_total, uint32_t n_step_cap, const int32_t* rays_alive, const float* rays_t,
                       const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                       const uint8_t* grid, const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                       const float* noises, uint32_t rows, ngp_stream_t stream);
/* ngp_march_rays_dev that also PUBLISHES the rows that can carry a sample in this iteration (rows_used: device word = min(rows, n_alive * n_step
 * padded by the marchers' rule); only those rows are zero-filled) for consumers that are launched for a stale bound and stop at the device-side
 * count (ngp_grid_encode_forward_sel, ngp_network_forward_rows).  rows_used == NULL: ngp_march_rays_dev. */
int ngp_march_rays_dev_rows(const int32_t* state, uint32_t alive_bound, uint32_t n_total, uint32_t n_step_cap, const int32_t* rays_alive, const float* rays_t,
                            const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                            const uint8_t* grid, const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas,
                            const float* noises, uint32_t rows, uint32_t* rows_used, ngp_stream_t stream);
int ngp_composite_rays_dev(const int32_t* state, uint32_t alive_bound, uint32_t n_total, uint32_t n_step_cap, float T_thresh, int32_t* rays_alive, float* rays_t,
                           const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum, float* depth, float* image,
                           ngp_stream_t stream);
int ngp_compact_rays_dev(const int32_t* state, uint32_t alive_bound, uint32_t n_total, uint32_t n_step_cap, uint32_t max_steps, const int32_t* rays_alive,
                         int32_t* out_alive, int32_t* out_state, void* workspace, ngp_stream_t stream);

/* EXTENSION (not in the reference): caller-defined per-sample channels in the inference loop -- the non-mutating companion of
 * ngp_composite_rays / ngp_composite_rays_dev.  Call it BEFORE that entry, on the same sample rows, alive list and stream: it reads the
 * weights_sum the compositor is about to advance and, for list entry n (index = rays_alive[n], rows s = n * n_step + step), runs the
 * compositor's own statements
 *   ws = weights_sum[index];  per step:  d0 = deltas[s,0], d0 == 0 ends the ray BEFORE anything of the row is read;
 *   alpha = 1 - exp(-sigmas[s] d0), T = 1 - ws, w = alpha T, ws += w;  out[index, c] += w feats[s, c]  (c = 0 .. C-1);  T < T_thresh ends the
 *   ray BEHIND the accumulation
 * in fp32 with an unfused multiply and add, in step order, starting from the out the caller passes: the result does not depend on how a
 * ray's samples are chunked into calls; with feats = rgbs (and out = image) it has the bits of the compositor's image, with a channel of
 * ones (out = weights_sum) those of its weights_sum.  Only out [N,C] fp32 is written -- rays_alive, weights_sum and the sample rows are
 * read, rows at or behind a ray's end are not.  feats [>= n_alive * n_step, C] of feat_dtype (NGP_F32 or NGP_F16; fp16 is converted at the
 * load: the bits of the fp32 call on the up-cast values), 1 <= C <= 256.  Deterministic: list entries are distinct rays, nothing crosses
 * lanes.  _dev: n_alive and n_step = max(min(n_total / n_alive, cap), 1) come from `state` as in ngp_composite_rays_dev (same n_total and
 * n_step_cap as the other calls of the iteration); entries beyond the device-side count do nothing.
 * C outside 1 .. 256, an unknown feat_dtype, n_step_cap > 1024 or a NULL tensor: NGP_ERR_INVALID.  n_alive == 0 / alive_bound == 0: nothing
 * is launched. */
int ngp_composite_rays_features(uint32_t n_alive, uint32_t n_step, float T_thresh, const int32_t* rays_alive, const float* sigmas,
                                const void* feats, const float* deltas, const float* weights_sum, uint32_t C, int feat_dtype,
                                float* out, ngp_stream_t stream);
int ngp_composite_rays_features_dev(const int32_t* state, uint32_t alive_bound, uint32_t n_total, uint32_t n_step_cap, float T_thresh,
                                    const int32_t* rays_alive, const float* sigmas, const void* feats, const float* deltas,
                                    const float* weights_sum, uint32_t C, int feat_dtype, float* out, ngp_stream_t stream);

/* n iterations of the eval loop (renderer.py:341-367: march_rays -> network -> composite_rays -> compaction of the alive list) issued by ONE
 * call -- EXTENSION: ngp_march_rays_dev -> ngp_grid_encode_forward_sched -> ngp_network_forward (inference, density scale
 * folded) -> ngp_composite_rays_dev -> ngp_compact_rays_dev per iteration, on the ping-pong alive lists / device state of the *_dev entry
 * points (iteration i works on state[(first_cur + i) & 1] and leaves the compacted list in the other one).  Launches are sized by `lanes`
 * and `rows` (host values: the caller's last known alive count); rows beyond the device-side count are zero rows, lanes beyond it idle.
 * `noises` (may be NULL) is handed to the first iteration of the call only.  Same kernels, arguments and order as the per-stage calls: the
 * image is the same, bit for bit.  Sample buffers xyzs / dirs [rows,3], deltas [rows,2], sigmas [rows], rgbs [rows,3] fp32 and enc
 * [L,rows,2] fp16 are caller-provided scratch; the network tensors are the fp16 copies (embeddings [n,2], w_sigma, w_color flat). */
typedef struct ngp_render_loop {
    int32_t* state;                 /* [2][2] {alive rays, steps marched} */
    int32_t* alive[2];
    float* rays_t; const float* rays_o; const float* rays_d; const float* nears; const float* fars; const uint8_t* grid; const float* noises;
    float* xyzs; float* dirs; float* deltas; void* enc; float* sigmas; float* rgbs;
    const void* embeddings; const int32_t* offsets; const float* level_cost_host; const void* w_sigma; const void* w_color;
    float* weights_sum; float* depth; float* image; void* compact_workspace;
    uint32_t* rows_used;            /* optional device word: the encoder / network launches stop at the rows the march of the same iteration emitted */
    uint32_t lanes, rows, n_total, n_step_cap, max_steps, cascade, grid_size;
    uint32_t L, H, gridtype, interp, num_layers_sigma, num_layers_color;
    int32_t align_corners;
    float bound, dt_gamma, T_thresh, S, density_scale;
} ngp_render_loop_t;
int ngp_render_iterations_dev(const ngp_render_loop_t* args, uint32_t n_iter, uint32_t first_cur, ngp_stream_t stream);

/* Empty-ray culling for the inference loop -- EXTENSION (no reference counterpart: renderer.py:330-333 starts every frame with all N rays
 * alive).  ngp_coarse_occupancy: per cascade a (H/4)^3 byte grid (x fastest), 1 when any voxel of the cell's 4^3 block or of one of its 26
 * neighbouring blocks is occupied (ngp_coarse_occupancy_bytes(C, H) bytes).  ngp_cull_rays: rays_alive[n] = n, or -1 for a ray whose segment
 * [near, far] provably (conservatively: half-cell sampling of the dilated grid, every cascade the marcher could select) meets no occupied
 * voxel -- such a ray would emit no sample, so dropping it from the initial alive list (ngp_compact_rays) leaves the image bit-identical.
 * Verdicts that do not depend on the grid: near >= far (the ray misses the box; near or far NaN included) gives -1.  With near < far a
 * DEGENERATE ray is KEPT, not judged: a zero direction, a direction with a NaN or infinite length, far = +inf, and a ray that is not through
 * after 4096 samples (e.g. near = 0, far = 2000 in a bound-1 box of 16^3).  Entries of rays_alive behind N are not written.  The verdicts
 * are pinned ray for ray by tests/test_gpu_occupancy.py against oracle/ngp_oracle.c orc_cull_rays, the coarse grid against
 * tests/occupancy_cases.py coarse_model. */
size_t ngp_coarse_occupancy_bytes(uint32_t C, uint32_t H);
int ngp_coarse_occupancy(const uint8_t* grid, uint32_t C, uint32_t H, uint8_t* coarse, ngp_stream_t stream);
int ngp_cull_rays(const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N, float bound, uint32_t C,
                  uint32_t H, const uint8_t* coarse, int32_t* rays_alive, ngp_stream_t stream);

/* composite_rays_train with NeRFRenderer.run_cuda's epilogue fused (renderer.py:316-318):
 *   image_out = image + (1 - weights_sum) * bg,  depth_out = clamp(depth - nears, 0) / (fars - nears)
 * bg_mode 0: off (= the reference op), 1: scalar background bg_scalar, 2: per-ray background bg [N,3].
 * The backward takes the gradient of image_out (and optionally of weights_sum, may be NULL when bg_mode != 0).
 * rows_used (backward, may be NULL): device scalar = number of sample rows the marcher handed out (first word of the
 * march_rays_train workspace).  When given, grad_sigmas / grad_rgbs may arrive uninitialised: the kernel zeroes every row it does not
 * write a gradient to (rows behind a ray's early termination, rows >= *rows_used); when NULL the caller pre-zeroes them (the
 * reference contract). */
int ngp_composite_rays_train_forward_ex(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                        uint32_t M, uint32_t N, float T_thresh, float* weights_sum, float* depth, float* image,
                                        int bg_mode, float bg_scalar, const float* bg, const float* nears, const float* fars,
                                        float* image_out, float* depth_out, ngp_stream_t stream);
int ngp_composite_rays_train_backward_ex(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                         const float* rgbs, const float* deltas, const int32_t* rays,
                                         const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                         float T_thresh, float* grad_sigmas, float* grad_rgbs, int bg_mode, float bg_scalar,
                                         const float* bg, const uint32_t* rows_used, ngp_stream_t stream);

/* EXTENSION of composite_rays_train_forward / _backward (raymarching.cu:501-577, 602-682) for geometry losses: the same compositing
 * (weights_sum, depth and image are the bits of ngp_composite_rays_train_forward) plus, per ray, the distortion of
 * loss.py::EffDistLoss on the compositor's own weights and distances,
 *   distortion = sum_ij w_i w_j |t_i - t_j| + 1/3 sum_i w_i^2 deltas[i,0],   t_i = sum_{j<=i} deltas[j,1],
 * and a backward that propagates the gradients of ALL four outputs -- depth included, which ngp_composite_rays_train_backward drops as
 * the reference does -- to sigmas and rgbs in one sweep.  distortion [N], written at row rays[n,0] like the others (0 for an empty ray
 * and for one whose samples do not fit M).  Backward: each of grad_weights_sum [N], grad_depth [N], grad_image [N,3], grad_distortion
 * [N] may be NULL (= zero); weights_sum, depth, image, distortion are the forward's outputs; grad_sigmas [M] / grad_rgbs [M,3] are
 * written for composited rows only, the caller pre-zeroes them.  deltas and rays get no gradient. */
int ngp_composite_rays_train_geo_forward(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M,
                                         uint32_t N, float T_thresh, float* weights_sum, float* depth, float* image,
                                         float* distortion, ngp_stream_t stream);
int ngp_composite_rays_train_geo_backward(const float* grad_weights_sum, const float* grad_depth, const float* grad_image,
                                          const float* grad_distortion, const float* sigmas, const float* rgbs, const float* deltas,
                                          const int32_t* rays, const float* weights_sum, const float* depth, const float* image,
                                          const float* distortion, uint32_t M, uint32_t N, float T_thresh, float* grad_sigmas,
                                          float* grad_rgbs, ngp_stream_t stream);
/* fp64 twins of the two entries above (raymarching.cu:501-577, 602-682, loss.py::EffDistLoss in double, one lane per ray): the same
 * arguments with every floating tensor double, for torch.autograd.gradcheck */
int ngp_composite_rays_train_geo_forward_f64(const double* sigmas, const double* rgbs, const double* deltas, const int32_t* rays,
                                             uint32_t M, uint32_t N, float T_thresh, double* weights_sum, double* depth, double* image,
                                             double* distortion, ngp_stream_t stream);
int ngp_composite_rays_train_geo_backward_f64(const double* grad_weights_sum, const double* grad_depth, const double* grad_image,
                                              const double* grad_distortion, const double* sigmas, const double* rgbs,
                                              const double* deltas, const int32_t* rays, const double* weights_sum, const double* depth,
                                              const double* image, const double* distortion, uint32_t M, uint32_t N, float T_thresh,
                                              double* grad_sigmas, double* grad_rgbs, ngp_stream_t stream);

/* EXTENSION (not in the reference): composite arbitrary per-sample feature channels with the weights of composite_rays_train
 * (raymarching.cu:501-577: a ray with num == 0 or offset + num > M composites nothing, the sample that drives T below T_thresh is still
 * composited, alpha_i = 1 - exp(-sigma_i deltas[i,0]), T_i = prod_{j<i} (1 - alpha_j), w_i = alpha_i T_i):
 *   out[index, c] = sum_i w_i feats[offset + i, c],   c = 0 .. C-1,  1 <= C <= 256          (zeros for a ray that composites nothing)
 * sigmas [M], deltas [M,2], out [N,C] fp32; feats [M,C] of feat_dtype (NGP_F32 or NGP_F16; fp16 is converted at the load and
 * accumulated in fp32: the bits of the fp32 call on the up-cast values); rays [N,3] int32 (index, offset, num).
 * Backward, from grad_out [N,C] and the forward's out, with T_{i+1} the transmittance behind sample i:
 *   grad_feats[offset+i, c] = w_i grad_out[index, c]                                         (feat_dtype; fp16: the fp32 product rounded once)
 *   q_i = sum_c grad_out[index,c] feats[offset+i,c],   Q = sum_c grad_out[index,c] out[index,c]
 *   grad_sigmas[offset+i]   = deltas[offset+i,0] (T_{i+1} q_i - (Q - sum_{j<=i} w_j q_j))
 * grad_sigmas [M] fp32 / grad_feats [M,C] are written for composited rows only, the caller pre-zeroes them (the contract of
 * ngp_composite_rays_train_geo_backward).  deltas and rays get no gradient.  Deterministic: fixed-order reductions, no atomics.
 * C outside 1 .. 256, an unknown feat_dtype or a NULL tensor: NGP_ERR_INVALID.  N == 0 or M == 0: nothing is launched. */
int ngp_composite_rays_train_features_forward(const float* sigmas, const void* feats, const float* deltas, const int32_t* rays, uint32_t M,
                                              uint32_t N, uint32_t C, float T_thresh, int feat_dtype, float* out, ngp_stream_t stream);
int ngp_composite_rays_train_features_backward(const float* grad_out, const float* sigmas, const void* feats, const float* deltas,
                                               const int32_t* rays, const float* out, uint32_t M, uint32_t N, uint32_t C, float T_thresh,
                                               int feat_dtype, float* grad_sigmas, void* grad_feats, ngp_stream_t stream);
/* fp64 twins of the two entries above (one lane per ray): the same arguments with every floating tensor double and no feat_dtype, for
 * torch.autograd.gradcheck */
int ngp_composite_rays_train_features_forward_f64(const double* sigmas, const double* feats, const double* deltas, const int32_t* rays,
                                                  uint32_t M, uint32_t N, uint32_t C, float T_thresh, double* out, ngp_stream_t stream);
int ngp_composite_rays_train_features_backward_f64(const double* grad_out, const double* sigmas, const double* feats, const double* deltas,
                                                   const int32_t* rays, const double* out, uint32_t M, uint32_t N, uint32_t C,
                                                   float T_thresh, double* grad_sigmas, double* grad_feats, ngp_stream_t stream);

/* The image-space middle of one TRAINING iteration in one launch (optional extension; what the four calls
 * ngp_composite_rays_train_forward_ex -> ngp_pipeline_mse_loss -> ngp_composite_rays_train_backward_ex -> ngp_pipeline_rgb_backward
 * compute, expression for expression: raymarching.cu:501-577 forward, renderer.py:316-318 finish, nerf/utils.py:516,557 loss,
 * raymarching.cu:602-682 backward, the sigmoid of network_ff.py:72 backward).  One wavefront per ray.
 *   in : sigmas [M], rgbs [M,3], deltas [M,2] fp32, rays [N,3] int32 (index, offset, count), bg as in the _ex calls (bg_mode 1 or 2),
 *        nears / fars [N], target [N,3] fp32, loss_scale (device scalar, NULL = 1)
 *   out: weights_sum [N], image_out [N,3], depth_out [N] (finished), loss [1] = mean((image_out - target)^2) (deterministic),
 *        grad_sigmas [M] fp32, grad_out16 [M,16] fp16 (columns 0..2 = dL/d(colour-net output) * loss_scale, rest 0) -- both may arrive
 *        uninitialised, every row is written (zeros where no gradient flows)
 *   loss may be NULL: the sum is then left to the caller (ngp_grid_encode_backward_checked_slabs carries it); ray_err [N] holds the per-ray squared errors.
 *   ray_err [N] fp32: scratch.  march_workspace: the workspace ngp_march_rays_train_ex filled for these rays, all
 *        ngp_march_rays_train_workspace_bytes(N) bytes of it (word 0 = rows handed out, word 1 and the 32 words at its end, 128 bytes
 *        apart = tickets that call leaves at 0 and this one returns to 0).  march_workspace_bytes: the size of that buffer -- a call with fewer
 *        than ngp_march_rays_train_workspace_bytes(N) bytes is refused (the group tickets sit at its end). */
int ngp_composite_train_loss_backward(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M,
                                      uint32_t N, float T_thresh, int bg_mode, float bg_scalar, const float* bg, const float* nears,
                                      const float* fars, const float* target, const float* loss_scale, float* weights_sum,
                                      float* image_out, float* depth_out, float* loss, float* ray_err, float* grad_sigmas,
                                      void* grad_out16, void* march_workspace, size_t march_workspace_bytes, ngp_stream_t stream);
/* ngp_composite_train_loss_backward with the geometry terms of ngp_composite_rays_train_geo_forward / _backward in the loss (optional
 * extension, one launch, the same contract for grad_sigmas / grad_out16 / ray_err / loss / the tickets / march_workspace_bytes), N rays:
 *   L = mean((image_out - target)^2) + lambda_distortion * mean_n(dist_n / span_n) + lambda_depth * mean_n(m_n * (d_n - z_n)^2),
 *   span_n = max(fars_n - nears_n, FLT_MIN);  dist_n, d_n: the raw distortion and depth of ngp_composite_rays_train_geo_forward
 *   in : ... as above, then after target: lambda_distortion, lambda_depth (finite, >= 0), target_depth z [N] (may be NULL only when
 *        lambda_depth == 0), depth_weight m [N] (NULL = 1), both read at row rays[n,0] like target
 *   out: ... as above, then after depth_out: depth_raw [N] (= d) and distortion [N] (= dist / span, the value the renderer returns)
 * The gradients are those of the chain geo_forward -> ngp_pipeline_mse_loss + the per-ray gradients of the two terms -> geo_backward ->
 * ngp_pipeline_rgb_backward, bit for bit; with both lambdas 0 every output of ngp_composite_train_loss_backward has the same bits.  ray_err
 * [N] holds the per-ray squared error + 3 x the ray's two terms, so that sum / (3 N) -- here or in the carrying launch -- is L.  A ray
 * without rows contributes its terms to L (depth 0, distortion 0) and no gradient.  N == 0: no-op. */
int ngp_composite_train_geo_loss_backward(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M,
                                          uint32_t N, float T_thresh, int bg_mode, float bg_scalar, const float* bg, const float* nears,
                                          const float* fars, const float* target, float lambda_distortion, float lambda_depth,
                                          const float* target_depth, const float* depth_weight, const float* loss_scale,
                                          float* weights_sum, float* image_out, float* depth_out, float* depth_raw, float* distortion,
                                          float* loss, float* ray_err, float* grad_sigmas, void* grad_out16, void* march_workspace,
                                          size_t march_workspace_bytes, ngp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * freqencoder       (reference: freqencoder/src/freqencoder.h:6-10, bindings.cpp:5-8) -- SURVEY.md 8(f).3; fp32, *_f64 twins.
 * outputs [B,C], C = D + 2*D*deg: x | per frequency f: sin(2^f x_d) for all d, then cos(2^f x_d) for all d.
 * --------------------------------------------------------------------------------------------- */
/* replaces freq_encode_forward (freqencoder.cu:97-111) */
int ngp_freq_encode_forward(const float* inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C, float* outputs,
                            ngp_stream_t stream);
/* replaces freq_encode_backward (freqencoder.cu:114-131): grad [B,C], outputs [B,C] (saved), grad_inputs [B,D] overwritten */
int ngp_freq_encode_backward(const float* grad, const float* outputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                             float* grad_inputs, ngp_stream_t stream);
/* EXTENSION of freq_encode_forward (freqencoder.cu:97-111) to float64: the same kernel on double, cos as sin(. + pi/2) in double */
int ngp_freq_encode_forward_f64(const double* inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C, double* outputs,
                                ngp_stream_t stream);
/* EXTENSION of freq_encode_backward (freqencoder.cu:114-131) to float64 */
int ngp_freq_encode_backward_f64(const double* grad, const double* outputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                                 double* grad_inputs, ngp_stream_t stream);
/* EXTENSION, the backward of freq_encode_backward (freqencoder.cu:114-131) for a loss on grad_inputs (torch.autograd.grad(...,
 * create_graph=True)): u [B,D] = d loss / d grad_inputs; grad [B,C] and outputs [B,C] as the first backward saw them.
 *   grad_grad    [B,C]  identity block u_d; sin slot 2^f u_d cos[f,d]; cos slot -2^f u_d sin[f,d]      (NULL: not computed)
 *   grad_inputs2 [B,D]  -u_d sum_f 4^f (g_sin[f,d] sin[f,d] + g_cos[f,d] cos[f,d])                       (NULL: not computed)
 * Both are overwritten, deterministic, no atomics.  dtype F32 or F64 (all five tensors).  A wrong C, a dtype other than F32 / F64, a
 * NULL grad / outputs / u: NGP_ERR_INVALID (B == 0 is a no-op). */
int ngp_freq_encode_backward_backward(const void* grad, const void* outputs, const void* u, uint32_t B, uint32_t D, uint32_t deg,
                                      uint32_t C, void* grad_grad, void* grad_inputs2, int dtype, ngp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused optimizer + loss-scaling step -- EXTENSION: replaces torch.optim.Adam + GradScaler.step/update
 * (main_nerf.py:132, nerf/utils.py:557-560) for up to 8 tensors per call.  grads[k] holds the loss-scaled gradient, fp16 when
 * grad_is_half[k] & 1 (the buffer grid_encode_backward / ffmlp_backward wrote) else fp32, and is ZEROED by the call -- unless
 * grad_is_half[k] & 2: the producer of that buffer overwrites ALL of it every step (ngp_grid_encode_backward_checked_slabs with
 * overwrite_table), so it is left as it is (and a skipped step does not touch the tensor at all); params_fp16[k]
 * (optional, may be NULL per tensor or as a whole) receives the fp16 copy of the updated weights.
 * state = device float[8], 16-byte aligned: {loss scale, growth tracker, found_inf, Adam step count, lr multiplier, table parity (ngp_table_adam_t), ticket of
 * ngp_optim_adam_small_commit (0 between launches), scale_dead (sticky: set by COMMIT once the loss scale has underflowed -- 1 / scale not
 * finite -- after which every step is skipped: the run is dead and says so)};
 * no host sync.
 * grad_mult: extra factor on the gradients (1 / world_size after a SUM all-reduce).  A step over more than 8 tensors uses
 * ngp_optim_adam_step_ex below (phases), which keeps "a non-finite gradient anywhere skips the whole step" across calls; for
 * compatibility growth_interval < 0 here still means "CHECK + UPDATE of this chunk, no COMMIT".
 * A loss scale that has underflowed (1 / scale not finite in fp32: 0 or a denormal, after a long run of overflowing steps) counts as an
 * overflow of its own: UPDATE skips, COMMIT backs off -- GradScaler's unscale-then-check order, so that a zero gradient is never
 * multiplied by 1 / 0 into the weights. */
int ngp_optim_adam_step(int count, const uint64_t* n, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                        void* const* grads, void* const* params_fp16, const int* grad_is_half, const float* lr, float beta1,
                        float beta2, float eps, float grad_mult, float growth_factor, float backoff_factor, float growth_interval,
                        float* state, ngp_stream_t stream);

/* The same step in phases, for parameter sets of more than 8 tensors and for the data-parallel sharded update: CHECK sweeps the
 * gradients of this call's tensors into found_inf, UPDATE applies Adam (or skips) to them, COMMIT updates the loss scale and the step
 * count once (count may be 0 for a COMMIT-only call).  A caller with several chunks issues CHECK for every chunk, then UPDATE for every
 * chunk, then COMMIT -- a non-finite gradient anywhere then skips the step everywhere, as GradScaler.step does.
 * ema / ema_one_minus_decay (optional: NULL / 0): exponential moving average of the parameters in the same sweep,
 * ema[k] -= ema_one_minus_decay * (ema[k] - params[k]) on the updated parameters -- torch_ema's ExponentialMovingAverage.update()
 * (the reference Trainer's `ema`, nerf/utils.py:388-391,760-761,891-892); the caller computes the effective decay
 * min(decay, (1 + num_updates) / (10 + num_updates)). */
#define NGP_OPT_PHASE_CHECK 1u
#define NGP_OPT_PHASE_UPDATE 2u
#define NGP_OPT_PHASE_COMMIT 4u
/* with COMMIT: a step that stands also flips state[5], the parity of a speculatively updated table (ngp_table_adam_t) */
#define NGP_OPT_PHASE_FLIP 8u
int ngp_optim_adam_step_ex(int count, const uint64_t* n, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                           void* const* grads, void* const* params_fp16, const int* grad_is_half, const float* lr, float beta1,
                           float beta2, float eps, float grad_mult, float growth_factor, float backoff_factor, float growth_interval,
                           float* state, float* const* ema, float ema_one_minus_decay, uint32_t phases, ngp_stream_t stream);
/* The rest of a step whose hash table was updated inside the grid backward (ngp_table_adam_t): Adam (same rule, same arithmetic, the
 * skip-as-a-whole verdict read from state[2]) on what is left -- the few SMALL tensors (the two MLPs' weights, updated in place) and,
 * table != NULL, the first table_prefix_params parameters of the double-buffered table (the dense levels: read from buffer set state[5]
 * with the stored fp16 gradient table_grad_fp16, written to the other set; nothing is written when the step is skipped) -- followed by
 * the COMMIT of the loss scale / step count and, flip_parity != 0, the parity flip that makes the speculatively written table current.
 * ONE launch of a few workgroups; the last one to finish (a ticket in state[6]) commits.  count may be 0.  At most 8 tensors and 4 M
 * parameters in total; table_prefix_params a multiple of 4. */
struct ngp_table_adam;
int ngp_optim_adam_small_commit(int count, const uint64_t* n, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                                void* const* grads, void* const* params_fp16, const int* grad_is_half, const float* lr, float beta1,
                                float beta2, float eps, float grad_mult, float growth_factor, float backoff_factor, float growth_interval,
                                float* state, int flip_parity, const struct ngp_table_adam* table, const void* table_grad_fp16,
                                uint64_t table_prefix_params, ngp_stream_t stream);
/* Data-parallel sharded update (one process per GPU, reduce-scatter -> Adam on 1/world -> all-gather; the reference's dormant DDP hook,
 * nerf/utils.py:364-366, all-reduces everything): the global "skip this step" verdict without a collective of its own.
 * ngp_optim_poison_shards: when state[2] (found_inf of THIS rank's local gradient) is set, writes NaN into element 0 of each of the `shards`
 * shards (of `payload` fp16 elements) of the flat gradient, BEFORE the reduce-scatter; ngp_optim_shard_verdict: AFTER it, sets state[2] when
 * element 0 of this rank's averaged shard is not finite, and (flat_grad_fp16 != NULL) takes the poison out of the flat buffer again -- a
 * poisoned element inside padding would otherwise survive when the producers overwrite and nobody zeroes.  Both are single tiny launches,
 * graph-capturable. */
int ngp_optim_poison_shards(void* flat_grad_fp16, uint32_t shards, uint64_t payload, const float* state, ngp_stream_t stream);
int ngp_optim_shard_verdict(const void* shard_grad_fp16, float* state, void* flat_grad_fp16, uint32_t shards, uint64_t payload,
                            ngp_stream_t stream);
/* torch_ema's update() on its own (the Trainer calls it once per epoch): ema[k] -= one_minus_decay * (ema[k] - params[k]), up to 8
 * tensors per call */
int ngp_optim_ema_update(int count, const uint64_t* n, float* const* params, float* const* ema, float one_minus_decay, ngp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * native command list: record the stream operations of a chain of entries once, replay them from C
 * ---------------------------------------------------------------------------------------------
 * Between ngp_cmdlist_begin and ngp_cmdlist_end every stream operation (kernel launch, memset, copy) that the entries of this header issue
 * ON THE CALLING THREAD is appended to the list -- function, grid, block, dynamic LDS and a private copy of every kernel argument -- and is
 * still issued on the stream it was given (a surrounding stream capture sees what it saw before).  ngp_cmdlist_replay issues the recorded
 * operations in order on `stream`; the caller keeps every buffer the recorded arguments point to alive for as long as the list is replayed.
 * A list is recorded once.  An entry that fails while a list records leaves the list unusable (replay refuses it).
 * Marks: ngp_cmdlist_mark(list, id, after) names a position -- after < 0: the current end (while recording: behind what was issued so
 * far), else behind the first `after` operations; a replay records a list-owned event (timing disabled) on its stream there, and
 * ngp_cmdlist_wait_mark makes another stream wait for that event of the most recent replay.
 * Refused with NGP_ERR_INVALID before any device work: a NULL or destroyed list (every entry, a second destroy included); begin while a
 * recording is open on the thread; end without begin; replay / wait_mark / destroy of a list that is still recording; replay / wait_mark
 * of an empty or unusable list; wait_mark of a mark id that was never recorded, or before the first replay that records it. */
int ngp_cmdlist_create(void** out_list);
int ngp_cmdlist_begin(void* list);
int ngp_cmdlist_mark(void* list, uint32_t mark_id, int after);
int ngp_cmdlist_end(void* list);
int ngp_cmdlist_count(const void* list, uint32_t* out_count);
/* entry `index` by name: the kernel's symbol (or "memset" / "memcpy"), NUL-terminated and cut to out_bytes */
int ngp_cmdlist_entry_name(const void* list, uint32_t index, char* out_name, uint32_t out_bytes);
int ngp_cmdlist_replay(void* list, ngp_stream_t stream);
int ngp_cmdlist_wait_mark(void* list, uint32_t mark_id, ngp_stream_t stream);
int ngp_cmdlist_destroy(void* list);

/* ---------------------------------------------------------------------------------------------
 * Camera-pose gradients through the training rays -- EXTENSION (csrc/ray_gradient.hip).  ctypes-only: the compiled
 * _raymarching / _gridencoder tables stay the reference's.
 * ---------------------------------------------------------------------------------------------
 * The marcher's sample parameters are constants: a sample of ray n is x_i = clamp(o_n + t_i d_n, -bound, bound), and t_i, deltas and the
 * choice of samples do not depend on the pose.  m_ij = 1 if |x_ij| < bound else 0 (a clamped coordinate passes no gradient).  rays [N,3]
 * int32 = (ray index n, first sample, sample count) as ngp_march_rays_train leaves it; a row with count 0, first + count > M or n >= N owns
 * no samples.  Every sum is taken in a fixed order without float atomics: the same bits from every launch, whatever the order of the rows
 * of `rays`.  All entries: bound > 0; a NULL or misaligned required pointer, an unsupported shape: NGP_ERR_INVALID before any device work;
 * M == 0 or N == 0: NGP_OK, no kernel, the outputs zeroed. */
/* extends march_rays_train (raymarching.cu:345-460), which keeps t to itself: ts [M] recovered from its output,
 * t_i = sum_j m_ij d_j (x_ij - o_j) / sum_j m_ij d_j^2 (0 when the denominator is 0; formed in double, rounded once).  xyzs [M,3], rays_o /
 * rays_d [N,3]; rows no ray owns are 0. */
int ngp_ray_sample_ts(const float* xyzs, const float* rays_o, const float* rays_d, const int32_t* rays, uint32_t M, uint32_t N, float bound,
                      float* ts, ngp_stream_t stream);
int ngp_ray_sample_ts_f64(const double* xyzs, const double* rays_o, const double* rays_d, const int32_t* rays, uint32_t M, uint32_t N,
                          float bound, double* ts, ngp_stream_t stream);
/* the sample statement of march_rays_train (raymarching.cu:433-441) on given ts: xyzs [M,3] = clamp(fma(t, d, o), -bound, bound), dirs [M,3]
 * = d; rows no ray owns are zero */
int ngp_ray_points_forward(const float* rays_o, const float* rays_d, const float* ts, const int32_t* rays, uint32_t M, uint32_t N, float bound,
                           float* xyzs, float* dirs, ngp_stream_t stream);
int ngp_ray_points_forward_f64(const double* rays_o, const double* rays_d, const double* ts, const int32_t* rays, uint32_t M, uint32_t N,
                               float bound, double* xyzs, double* dirs, ngp_stream_t stream);
/* its backward, one wavefront per ray like ngp_composite_rays_train_backward:
 *   grad_rays_o[n,j] = sum_i m_ij grad_xyzs[i,j]
 *   grad_rays_d[n,j] = sum_i t_i m_ij grad_xyzs[i,j] + sum_i grad_dirs[i,j] + (J_SH4(d_n)^T sum_i grad_sh16[i, 0:16])_j
 * grad_dirs [M,3] (optional) and grad_sh16 [M,32] fp16 (optional, 16-byte aligned: the colour net's input gradient of
 * ngp_ffmlp_backward_ex, columns 0..15 = dL/dSH4(d) on the raw direction as ngp_pipeline_mid_forward evaluates it) may be NULL.  Every
 * ray's row of grad_rays_o / grad_rays_d [N,3] is written (zeros for a ray without samples); rows of the per-sample tensors that no ray
 * owns are never read. */
int ngp_ray_points_backward(const float* grad_xyzs, const float* grad_dirs, const void* grad_sh16, const float* xyzs, const float* ts,
                            const float* rays_d, const int32_t* rays, uint32_t M, uint32_t N, float bound, float* grad_rays_o,
                            float* grad_rays_d, ngp_stream_t stream);
int ngp_ray_points_backward_f64(const double* grad_xyzs, const double* grad_dirs, const double* xyzs, const double* ts, const double* rays_d,
                                const int32_t* rays, uint32_t M, uint32_t N, float bound, double* grad_rays_o, double* grad_rays_d,
                                ngp_stream_t stream);
/* extends kernel_input_backward (gridencoder.cu:343-369) to the fused path, which has no dy_dx: grad_enc [L][M][2] fp16 planar (what
 * ngp_ffmlp_backward_ex writes with NGP_FF_DX_PLANAR), xyzs [M,3] fp32, the fp16 table and offsets of ngp_grid_encode_forward_ex ->
 *   grad_xyzs[i,j] = 1 / (2 bound) * sum_l sum_c grad_enc[l,i,c] dy_dx[i,l,j,c]       (bound == 0: unit coordinates, factor 1)
 * with dy_dx what ngp_grid_encode_forward defines (level scale * phi' * the weights of the other two coordinates * the difference of the
 * two table values), recomputed from the table in fp32 instead of stored and read back in fp16; levels summed in order, a point outside
 * the unit cube gets zeros.  D = 3, C = 2, dtype NGP_F16 only -- anything else: NGP_ERR_INVALID. */
int ngp_grid_input_gradient(const void* grad_enc, const float* xyzs, const void* embeddings, const int32_t* offsets, uint32_t M, uint32_t D,
                            uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                            float bound, float* grad_xyzs, ngp_stream_t stream);
/* the backward of ngp_rays_from_pixels in the poses (intrinsics, W, inds, inds_batch_stride as in the forward; dcam, the normalised pinhole
 * direction, is recomputed per pixel): grad_rays_o, grad_rays_d [B,N,3] -> grad_poses [B,4,4],
 *   grad_poses[b,r,3] = sum_n grad_rays_o[b,n,r],  grad_poses[b,r,c] = sum_n grad_rays_d[b,n,r] dcam[n,c]  (r, c < 3),  row 3 = 0 */
int ngp_rays_from_pixels_backward(const float* grad_rays_o, const float* grad_rays_d, uint32_t B, float fx, float fy, float cx, float cy,
                                  uint32_t W, const int64_t* inds, uint32_t inds_batch_stride, uint32_t N, float* grad_poses,
                                  ngp_stream_t stream);

/* ---- error-map ray sampling (csrc/error_map.hip) ----
 * replaces the error-map branch of get_rays (nerf/utils.py:85-106: torch.multinomial(error_map, N, replacement=False) over the res x res
 * map, then a uniform offset inside each drawn cell) by ONE launch that uses no torch generator: per image b, N distinct cells drawn by
 * successive sampling without replacement proportional to error_map[b] (the exponential race torch.multinomial itself runs), refined to
 * pixels of the H x W frame.  All integer arithmetic mod 2^32:
 *   s = seed + (seed_dev ? *seed_dev : 0)        seed_dev: one device word read by the kernel (e.g. the optimizer's step count)
 *   mix(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16       (the finaliser of the marcher's seeded noise)
 *   word(i, b, k) = mix(mix((i * 0x9E3779B9) ^ (s * 0x85EBCA6B + 0x27D4EB2F)) ^ (b * 0xC2B2AE35 + k * 0x165667B1 + 0x27D4EB2F))
 *   u_i = (float)(((word(i, b, 0) >> 9) << 1) | 1) * 2^-24                                   (exact, strictly inside (0, 1))
 *   key_i = isfinite(w_i) && w_i > 0 ? -logf(u_i) / w_i : +inf                               (w = error_map[b]; fp32)
 * The drawn set is the N cells smallest by (key bits as uint32, cell index), written in ASCENDING cell order: exactly N distinct cells
 * whatever the map holds; zero, negative, NaN and inf weights are drawn only when fewer than N cells are drawable, lowest index first.
 * Refinement (plain fp32, no fma): cell_h = (float)H / (float)res, cell_w = (float)W / (float)res,
 *   r = (word(i, b, 1) >> 8) * 2^-24, c = (word(i, b, 2) >> 8) * 2^-24,
 *   row = min((uint32)((float)(i / res) * cell_h + r * cell_h), H - 1), col = min((uint32)((float)(i % res) * cell_w + c * cell_w), W - 1)
 * inds [B,N] = row * W + col, inds_coarse [B,N] = i (both int64, as torch indices).  Optional outputs: keys_out [B, res * res] (every
 * cell's key), n_drawable [B] (cells with a finite positive weight: a caller can check without a fault or a synchronisation).
 * One workgroup per image, keys in registers, radix select over an LDS histogram: no global atomics, no workspace, no host read-back
 * (capturable).  NGP_ERR_INVALID before any device work: NULL error_map / inds / inds_coarse, res outside 1 .. 128, N > res * res,
 * H == 0, W == 0 or H * W >= 2^31.  B == 0 or N == 0: nothing is launched. */
int ngp_error_map_draw(const float* error_map, uint32_t B, uint32_t res, uint32_t N, uint32_t H, uint32_t W, uint32_t seed,
                       const uint32_t* seed_dev, int64_t* inds, int64_t* inds_coarse, float* keys_out, uint32_t* n_drawable,
                       ngp_stream_t stream);
/* replaces the Trainer's error-map update (nerf/utils.py, train_step's error-map branch: error = loss.mean(-1) per ray, gather the
 * cells' old values, ema_error = 0.1 * old + 0.9 * error, scatter_ back) for one image's row error_map_row [n_cells]: for each ray n with
 * c = inds_coarse[n] in [0, n_cells), e_k = image[n,k] - target[n,k] (image, target [N,3] fp32),
 *   err = ((e0 * e0 + e1 * e1) + e2 * e2) / 3.0f,   error_map_row[c] = keep * error_map_row[c] + take * err     (plain fp32)
 * A cell index out of range skips that ray; cells that are not named keep their bits; a cell named more than once receives an
 * unspecified one of its candidates (as scatter_ does; ngp_error_map_draw never names a cell twice).  NULL tensor: NGP_ERR_INVALID. */
int ngp_error_map_update(float* error_map_row, const int64_t* inds_coarse, const float* image, const float* target, uint32_t N,
                         uint32_t n_cells, float keep, float take, ngp_stream_t stream);

/* ---- signed-distance fields: NeuS's section opacity as a density (csrc/sdf_sigmas.hip) ----
 * NeuS (Wang et al. 2021; models/renderer.py) renders an SDF sample with the opacity
 *   alpha = clip((prev - next + eps) / (prev + eps), 0, 1),   prev = sigmoid(inv_s (sdf - h)),  next = sigmoid(inv_s (sdf + h)),  eps = 1e-5
 *   c = dirs . normals,   ic = -(relu(0.5 - 0.5 c) (1 - cos_anneal) + relu(-c) cos_anneal)  (<= 0),   h = 0.5 ic d0,   d0 = deltas[i,0]
 * Every compositor of this library takes a density and forms alpha = 1 - exp(-sigma * deltas[i,0]) itself (raymarching.cu:501-577), so the
 * entry returns the density that reproduces NeuS's alpha, in the form that has neither the prev - next nor the 1 - alpha cancellation
 * (1 - alpha = next / (prev + eps) exactly; h <= 0 gives next <= prev, the clip is never active):
 *   x = log(prev + eps) + softplus(-inv_s (sdf + h))   (= -log(1 - alpha)),     sigma = min(x, 15) / d0,     sigma = 0 where d0 == 0
 * The cap 15 is the bound of trunc_exp: a sample deep inside the surface ends the ray (1 - alpha = 3.1e-7) instead of producing inf.
 * sdf [M], normals [M,3] (the SDF's gradient, not normalised), dirs [M,3], deltas [M,2] (only column 0 is read, as one 8-byte load),
 * inv_s: ONE device float, read by the kernels; cos_anneal: host float in [0, 1]; sigmas [M].  One lane per row, one launch.
 * Backward, from grad_sigmas [M], recomputing the forward terms: with P = prev, A = P (1 - P) / (P + eps), B = 1 - next, gx = grad_sigmas / d0
 *   grad_sdf = gx inv_s (A - B),   dL/dh = -gx inv_s (A + B),   dh/dc = 0.5 d0 (0.5 (1 - cos_anneal) [c < 1] + cos_anneal [c < 0])
 *   grad_normals = dL/dh dh/dc dirs,   grad_dirs = dL/dh dh/dc normals  (grad_dirs may be NULL: not written),
 *   grad_inv_s[0] = sum_i gx_i (A_i (sdf_i - h_i) - B_i (sdf_i + h_i))
 * EVERY row of grad_sdf / grad_normals / grad_dirs is written: zeros for rows with d0 == 0 and for capped rows (x >= 15: the derivative
 * of min).  deltas gets no gradient.  grad_inv_s is summed in double in a fixed order without atomics -- an xor tree per wave, the waves of
 * a workgroup in order into partials[workgroup] (the workspace), then one workgroup adds the partials (thread t: t, t + 256, ... in index
 * order; the same wave / workgroup order) and rounds once; the grid is cdiv(M, 256) whatever the data: the same bits on every run.
 * workspace: ngp_sdf_sigmas_workspace_bytes(M) bytes (monotone in M), 8-byte aligned, contents irrelevant before and after.
 * NGP_ERR_INVALID before any device work: cos_anneal outside [0, 1]; for M > 0 a NULL tensor (other than grad_dirs), M > 2^31, a NULL or
 * short workspace.  M == 0: nothing is launched and nothing is written (the caller provides grad_inv_s = 0). */
size_t ngp_sdf_sigmas_workspace_bytes(uint32_t M);
int ngp_sdf_sigmas_forward(const float* sdf, const float* normals, const float* dirs, const float* deltas, const float* inv_s, uint32_t M,
                           float cos_anneal, float* sigmas, ngp_stream_t stream);
int ngp_sdf_sigmas_backward(const float* grad_sigmas, const float* sdf, const float* normals, const float* dirs, const float* deltas,
                            const float* inv_s, uint32_t M, float cos_anneal, float* grad_sdf, float* grad_normals, float* grad_dirs,
                            float* grad_inv_s, void* workspace, size_t workspace_bytes, ngp_stream_t stream);
/* fp64 twins (csrc/fp64.hip: the same kernel source instantiated for double): every floating tensor double, cos_anneal still a float; for
 * torch.autograd.gradcheck */
int ngp_sdf_sigmas_forward_f64(const double* sdf, const double* normals, const double* dirs, const double* deltas, const double* inv_s,
                               uint32_t M, float cos_anneal, double* sigmas, ngp_stream_t stream);
int ngp_sdf_sigmas_backward_f64(const double* grad_sigmas, const double* sdf, const double* normals, const double* dirs, const double* deltas,
                                const double* inv_s, uint32_t M, float cos_anneal, double* grad_sdf, double* grad_normals, double* grad_dirs,
                                double* grad_inv_s, void* workspace, size_t workspace_bytes, ngp_stream_t stream);

/* ---- mesh extraction: naive surface nets and the occupancy-culled lattice (csrc/surface_nets.hip) ----
 * Replaces the reference's save_mesh (nerf/utils.py: a dense torch volume, then mcubes / trimesh on the host).  Surface nets: one vertex per
 * sign-changing cell, one quad per sign-changing lattice edge -- no case table, an indexed mesh with shared vertices, fully deterministic.
 * Volume and sign: volume f[z][y][x], fp32, contiguous, nx, ny, nz >= 2, nx * ny * nz < 2^31.  s = f - level (inside_below != 0, as for an
 *   SDF: s = level - f).  A lattice point is inside iff s > 0; NaN and s == 0 count as outside.
 * Cells and vertices: cell (i, j, k), 0 <= i < nx - 1 (likewise j, k), spans the lattice points (i..i+1, j..j+1, k..k+1) and is active iff its
 *   eight corners are neither all inside nor all outside.  Vertices are numbered by an exclusive scan of the active flags in linear cell
 *   order (k (ny - 1) + j) (nx - 1) + i.  The vertex of an active cell is the mean of the crossing points of its sign-changing edges (3 to 12):
 *   on the edge from corner a to b = a + e_axis the crossing is a + t e_axis, t = s_a / (s_a - s_b) clamped to [0, 1], a non-finite t
 *   replaced by 0.5 (fp32).  The terms are added in cell-local coordinates (every term in [0, 1]^3) in a fixed order -- the x-edges, the
 *   y-edges, the z-edges, each four with the lower of the two other axes running fastest --, divided by their number, the integer cell
 *   coordinate is added, and the world position is fma(lattice, h, o) per axis.
 * Faces: axes (a, b, c) a cyclic triple of (x, y, z).  The lattice edge p -> p + e_a emits one quad iff it is interior, 1 <= p_b <= N_b - 2 and
 *   1 <= p_c <= N_c - 2, and inside(p) != inside(p + e_a).  Its corners are the vertices of the cells q0 = p - e_b - e_c, q1 = p - e_c,
 *   q2 = p, q3 = p - e_b; p inside: triangles (q0, q1, q2), (q0, q2, q3), else (q0, q3, q2), (q0, q2, q1): normals point from inside to
 *   outside.  Faces are ordered by (linear lattice index of p) * 3 + a, two triangles each, int32 indices.  A surface that leaves the box is
 *   left open there: nothing is emitted on boundary edges.
 * ngp_surface_nets_count: counts_dev[0] = V, counts_dev[1] = the number of triangles (device words; 0xFFFFFFFF: does not fit int32), and
 *   the scanned per-workgroup counts in the workspace.  ngp_surface_nets_emit, with the SAME volume, level, sense and workspace, after it on
 *   the stream: the flags are recomputed (no mask volume), the cell -> vertex map and vertices [V,3] are written, then -- a later launch --
 *   faces [F,3].  Every store is bounded by v_cap / f_cap (rows) on the device; the entry then reads the two counts back (it synchronises
 *   the stream: an export op, neither capturable nor recordable) and returns NGP_ERR_INVALID ("truncated") when a capacity is below its
 *   count -- a caller with stale counts gets a truncated mesh and an error, never a write past its buffers.  No atomics: the output order
 *   is the scans' order, the same bits on every run.
 * workspace: ngp_surface_nets_workspace_bytes(nx, ny, nz) bytes (monotone in each dimension; 0 for refused dimensions), 4-byte aligned: the
 *   int32 cell -> vertex map, one word per lattice point, and two scan words per workgroup of 256 lattice points.
 * NGP_ERR_INVALID before any device work: a NULL pointer, a dimension below 2, nx * ny * nz >= 2^31, a zero capacity (an empty mesh needs no
 *   emit). */
size_t ngp_surface_nets_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int ngp_surface_nets_count(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float level, int inside_below, void* workspace,
                           uint32_t* counts_dev, ngp_stream_t stream);
int ngp_surface_nets_emit(const float* volume, uint32_t nx, uint32_t ny, uint32_t nz, float level, int inside_below, float ox, float oy, float oz,
                          float hx, float hy, float hz, void* workspace, float* vertices, uint32_t v_cap, int32_t* faces, uint32_t f_cap,
                          ngp_stream_t stream);
/* the lattice points of the z-range [z0, z1) of an nx x ny x . lattice that lie near occupied space, compacted in lattice order: where an
 * extraction has to evaluate the field at all.  Point (i, j, k) has the world position fma(i, h, o) per axis and the linear index
 * (k ny + j) nx + i in the whole lattice (int32: nx * ny * z1 < 2^31).  Its cascade is the marcher's position term alone,
 * mip_exponent(max |x|, cascade - 1) (`lp` of probe_geom, raymarching.hip), its cell probe_geom's index statement at that cascade (positions
 * outside the cascade's box fall into its boundary cells).  The point is kept iff one of the (2 dilate + 1)^3 cells around its own cell at
 * that cascade has its bit set in `bitfield` (the layout of ngp_packbits; neighbour coordinates clamped to [0, grid_size - 1]); dilate in
 * [0, 4].  bitfield == NULL: every point is kept (bound, cascade, grid_size, dilate are not looked at).
 * Output: points [K,3] fp32, index [K] int32 and count_dev[0] = K, by the flag / scan / compact scheme of the extraction (no atomics, the same
 * bits on every run).  Stores are bounded by `capacity` (rows); K is the full count, so K > capacity tells the caller the output is cut.
 * workspace: ngp_lattice_points_workspace_bytes(nx, ny, z1 - z0) bytes, 4-byte aligned (one scan word per workgroup of 256 points) -- the
 * compaction across workgroups needs it like every scan of this library; contents irrelevant before and after.
 * NGP_ERR_INVALID before any device work: a NULL pointer (other than bitfield), an empty lattice or slab, nx * ny * z1 >= 2^31, zero capacity;
 * with a bitfield: bound <= 0, cascade outside [1, 8], grid_size not a power of two in [1, 1024], dilate > 4. */
size_t ngp_lattice_points_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz_slab);
int ngp_lattice_points(float ox, float oy, float oz, float hx, float hy, float hz, uint32_t nx, uint32_t ny, uint32_t z0, uint32_t z1,
                       const uint8_t* bitfield, float bound, uint32_t cascade, uint32_t grid_size, uint32_t dilate, void* workspace, float* points,
                       int32_t* index, uint32_t* count_dev, uint32_t capacity, ngp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NGP_HIP_H */
