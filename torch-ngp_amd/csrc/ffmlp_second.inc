// Second order of the fully fused MLP: the backward of ngp_ffmlp_backward's grad_inputs (DESIGN.md 3.7).  Included at the end of
// ffmlp.hip: it shares that file's weight images, fragment layout and weight-gradient kernel, and changes none of its kernels.
//
// With n = num_layers, h_l the stored post-activations, f(h) the factor of the first backward (act_backward_factor), f' its derivative
// with respect to h, d_l = e_l * f(h_l) the hidden gradients of the first backward and u = d loss / d grad_inputs:
//   tangent   p_0 = u;  q_l = p_{l-1} W_{l-1}^T,  p_l = q_l * f(h_l)  (l = 1..n);  d loss / d grad = p_n W_n^T
//   explicit  d loss / d W_l += d_{l+1}^T p_l  (l < n),  d loss / d W_n = grad^T p_n
//   implicit  (f' != 0 only)  r_l = q_l * e_l * f'(h_l);  t_n = r_n;  s_l = t_l * f(h_l);  d loss / d W_{l-1} += s_l^T h_{l-1};
//             t_{l-1} = s_l W_{l-1} (+ r_{l-1});  d loss / d inputs = t_0
// Every width runs these layered kernels (one matmul's image in LDS at a time); d_l, p_l, q_l and s_l cross memory as fp16 in the
// forward buffer's fragment order, everything else stays in fp32 registers.  The register-resident first backward uses its
// backward_buffer as slab scratch, so d_l is recomputed here with k_ffmlp_dgrad_layered.
namespace ngp {

// f'(y): the derivative of act_backward_factor with respect to the stored post-activation y
__device__ __forceinline__ float act_backward_factor_slope(uint32_t a, float y) {
    switch (a) {
        case ACT_EXP: return 1.0f;
        case ACT_SIGMOID: return 1.0f - 2.0f * y;
        case ACT_SQUAREPLUS: { const float s = y * K_ACT, d = s * s + 1.0f; return 2.0f * K_ACT * s / (d * d); }
        case ACT_SOFTPLUS: return K_ACT * __expf(-y * K_ACT);
        default: return 0.0f;  // ReLU, Sine, None: the first backward is linear in everything but the weights
    }
}
__host__ __device__ inline bool act_has_slope(uint32_t a) { return a == ACT_EXP || a == ACT_SIGMOID || a == ACT_SQUAREPLUS || a == ACT_SOFTPLUS; }

// Tangent pass: k_ffmlp_forward_layered<WIDTH, true> with u for the inputs and `* f(stored y)` for the activation.  Matmul m writes p_{m+1}
// (and q_{m+1} when q_buffer is given); the output-layer matmul, run only when grad_grad is given, writes d loss / d grad [B,16].
template <int WIDTH>
__global__ __launch_bounds__(FF_THREADS) void k_ffmlp_tangent_layered(const half_t* __restrict__ u, const half_t* __restrict__ weights,
                                                                      const half_t* __restrict__ forward_buffer, half_t* __restrict__ p_buffer,
                                                                      half_t* __restrict__ q_buffer, half_t* __restrict__ grad_grad,
                                                                      uint32_t n_tiles, uint32_t in_dim, uint32_t num_layers, uint32_t act) {
    constexpr int NIB = Shape<WIDTH>::NIB, NKB = Shape<WIDTH>::NKB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half8_t* img = reinterpret_cast<half8_t*>(smem);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = lane & 31, h = lane >> 5;
    const uint32_t in_kb = in_dim / 16;
    const size_t rows = (size_t)n_tiles * FF_TILE;
    const size_t layer_stride = (size_t)n_tiles * NKB * 64;  // half8 units
    const half8_t* fb = reinterpret_cast<const half8_t*>(forward_buffer);
    half8_t* pb = reinterpret_cast<half8_t*>(p_buffer);
    half8_t* qb = reinterpret_cast<half8_t*>(q_buffer);
    const half8_t* a = img + lane;
    const uint32_t matmuls = num_layers + (grad_grad ? 1u : 0u);
    for (uint32_t m = 0; m < matmuls; m++) {
        uint32_t first, count;
        fwd_matmul_range<WIDTH>(m, in_dim, num_layers, first, count);
        __syncthreads();  // the previous matmul's readers are done with the image
        build_forward_image<WIDTH>(img, weights, in_dim, num_layers, first, count);
        __syncthreads();
        for (uint32_t tile = blockIdx.x * FF_WAVES + wid; tile < n_tiles; tile += gridDim.x * FF_WAVES) {
            const size_t frag0 = (size_t)tile * NKB * 64 + lane;
            const half8_t* src = pb + (size_t)(m ? m - 1 : 0) * layer_stride + frag0;  // p_m (m >= 1 only)
            if (m == num_layers) {  // output layer: one 32-row block, rows 0..15 real
                float16_t o = zero16();
#pragma unroll
                for (int kb = 0; kb < NKB; kb++) o = mfma(a[kb * 64], src[kb * 64], o);
                half4_t lo, hi;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    lo[c] = (half_t)o[c];
                    hi[c] = (half_t)o[4 + c];
                }
                half_t* orow = grad_grad + ((size_t)tile * FF_TILE + n) * 16 + 4 * h;
                *reinterpret_cast<half4_t*>(orow) = lo;
                *reinterpret_cast<half4_t*>(orow + 8) = hi;
                continue;
            }
            float16_t acc[NIB];
#pragma unroll
            for (int ib = 0; ib < NIB; ib++) acc[ib] = zero16();
            if (m == 0) {
                const size_t srow = (size_t)tile * FF_TILE + n;
                for (uint32_t kb = 0; kb < in_kb; kb++) {
                    const half8_t x = load_features8(u, false, rows, srow, in_dim, 16 * kb + 8 * h);
#pragma unroll
                    for (int ib = 0; ib < NIB; ib++) acc[ib] = mfma(a[(ib * in_kb + kb) * 64], x, acc[ib]);
                }
            } else {
#pragma unroll
                for (int kb = 0; kb < NKB; kb++) {
                    const half8_t pk = src[kb * 64];
#pragma unroll
                    for (int ib = 0; ib < NIB; ib++) acc[ib] = mfma(a[(ib * NKB + kb) * 64], pk, acc[ib]);
                }
            }
            const half8_t* post = fb + (size_t)m * layer_stride + frag0;
            half8_t* dst_p = pb + (size_t)m * layer_stride + frag0;
#pragma unroll
            for (int kb = 0; kb < NKB; kb++) {
                const half8_t y = post[kb * 64];
                half8_t pf, qf;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float q = acc[kb >> 1][(kb & 1) * 8 + j];
                    pf[j] = (half_t)(q * act_backward_factor(act, (float)y[j]));
                    qf[j] = (half_t)q;
                }
                dst_p[kb * 64] = pf;
                if (qb) qb[(size_t)m * layer_stride + frag0 + kb * 64] = qf;
            }
        }
        __threadfence();
    }
}

// Second dgrad: k_ffmlp_dgrad_layered<WIDTH, false> with two accumulator chains over each weight image -- s_{l+1} W_l, and d_{l+1} W_l,
// which is e_l again (pass 0: grad W_n).  The epilogue forms r_l, t_l and s_l and stores s_l; the last pass (grad_inputs2 given) writes
// d loss / d inputs.  Only launched for activations with f' != 0.  One 32-row block at a time: 32 accumulator registers whatever the width.
template <int WIDTH>
__global__ __launch_bounds__(FF_THREADS) void k_ffmlp_dgrad2_layered(const half_t* __restrict__ grad, const half_t* __restrict__ weights,
                                                                     const half_t* __restrict__ forward_buffer, const half_t* __restrict__ d_buffer,
                                                                     const half_t* __restrict__ q_buffer, half_t* __restrict__ s_buffer,
                                                                     uint32_t n_tiles, uint32_t in_dim, uint32_t num_layers, uint32_t act,
                                                                     half_t* __restrict__ grad_inputs2) {
    constexpr int NIB = Shape<WIDTH>::NIB, NKB = Shape<WIDTH>::NKB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half8_t* img = reinterpret_cast<half8_t*>(smem);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = lane & 31, h = lane >> 5;
    const size_t layer_stride = (size_t)n_tiles * NKB * 64;
    const half8_t* fb = reinterpret_cast<const half8_t*>(forward_buffer);
    const half8_t* db = reinterpret_cast<const half8_t*>(d_buffer);
    const half8_t* qb = reinterpret_cast<const half8_t*>(q_buffer);
    half8_t* sb = reinterpret_cast<half8_t*>(s_buffer);
    const half8_t* a = img + lane;
    const uint32_t in_jb = (in_dim + 31) / 32;
    const bool with_dx = grad_inputs2 != nullptr;
    const uint32_t passes = num_layers + (with_dx ? 1u : 0u);
    // pass 0: grad W_n -> s_n; pass p (1..n-1): W_{n-p} under s_{n-p+1} and d_{n-p+1} -> s_{n-p}; pass n: s_1 W_0 -> d loss / d inputs
    for (uint32_t p = 0; p < passes; p++) {
        uint32_t first, count;
        if (p == 0) { first = 0; count = NIB; }
        else if (p < num_layers) { first = NIB + (p - 1) * NIB * NKB; count = NIB * NKB; }
        else { first = NIB + (num_layers - 1) * NIB * NKB; count = in_jb * NKB; }
        __syncthreads();
        build_backward_image<WIDTH>(img, weights, in_dim, num_layers, with_dx, first, count);
        __syncthreads();
        for (uint32_t tile = blockIdx.x * FF_WAVES + wid; tile < n_tiles; tile += gridDim.x * FF_WAVES) {
            const size_t srow = (size_t)tile * FF_TILE + n;
            const size_t frag0 = (size_t)tile * NKB * 64 + lane;
            const size_t above = (size_t)(p ? num_layers - p : 0) * layer_stride + frag0;  // s and d of layer n-p+1 (p >= 1)
            if (p == num_layers) {
                for (uint32_t ib = 0; ib < in_jb; ib++) {
                    float16_t dx = zero16();
#pragma unroll
                    for (int kb = 0; kb < NKB; kb++) dx = mfma(a[(ib * NKB + kb) * 64], sb[above + kb * 64], dx);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t f0 = 32 * ib + 8 * q + 4 * h;
                        if (f0 < in_dim) {
                            half4_t v = {(half_t)dx[4 * q], (half_t)dx[4 * q + 1], (half_t)dx[4 * q + 2], (half_t)dx[4 * q + 3]};
                            *reinterpret_cast<half4_t*>(grad_inputs2 + srow * in_dim + f0) = v;
                        }
                    }
                }
                continue;
            }
            half8_t sv[NKB], dv[NKB];
            half8_t dy = {};
            if (p == 0) {
                dy = *reinterpret_cast<const half8_t*>(grad + srow * 16 + 8 * h);
            } else {
#pragma unroll
                for (int kb = 0; kb < NKB; kb++) {
                    sv[kb] = sb[above + kb * 64];
                    dv[kb] = db[above + kb * 64];
                }
            }
            const size_t here = (size_t)(num_layers - 1 - p) * layer_stride + frag0;  // layer n-p
#pragma unroll
            for (int ib = 0; ib < NIB; ib++) {
                float16_t acc_s = zero16(), acc_e = zero16();
                if (p == 0) {
                    acc_e = mfma(a[ib * 64], dy, acc_e);
                } else {
#pragma unroll
                    for (int kb = 0; kb < NKB; kb++) {
                        const half8_t w = a[(ib * NKB + kb) * 64];
                        acc_s = mfma(w, sv[kb], acc_s);
                        acc_e = mfma(w, dv[kb], acc_e);
                    }
                }
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int kb = 2 * ib + e;
                    if (kb < NKB) {
                        const half8_t y = fb[here + kb * 64], q = qb[here + kb * 64];
                        half8_t s;
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const float yj = (float)y[j];
                            const float r = (float)q[j] * acc_e[8 * e + j] * act_backward_factor_slope(act, yj);
                            s[j] = (half_t)((acc_s[8 * e + j] + r) * act_backward_factor(act, yj));
                        }
                        sb[here + kb * 64] = s;
                    }
                }
            }
        }
        __threadfence();
    }
}

// workspace of ngp_ffmlp_backward_backward: four [num_layers, B, hidden] fp16 buffers in fragment order (d, p and, for activations with
// f' != 0, q and s), then two sets of WG_MAX_CHUNKS fp32 weight-gradient slabs (explicit and implicit terms)
struct SecondWorkspace {
    size_t d = 0, p = 0, q = 0, s = 0, slabs = 0, total = 0;
};
static SecondWorkspace second_workspace(uint32_t B, uint32_t in_dim, uint32_t hidden, uint32_t num_layers, uint32_t act) {
    SecondWorkspace w;
    const size_t layers = (((size_t)num_layers * B * hidden * sizeof(half_t)) + 255) / 256 * 256;
    w.d = 0;
    w.p = layers;
    w.total = 2 * layers;
    if (act_has_slope(act)) {
        w.q = w.total;
        w.s = w.total + layers;
        w.total += 2 * layers;
    }
    w.slabs = w.total;
    w.total += (size_t)2 * WG_MAX_CHUNKS * ff_param_count(in_dim, hidden, num_layers) * sizeof(float);
    return w;
}

static uint32_t layered_blocks(size_t lds, uint32_t n_tiles) {
    const uint32_t per_cu = (uint32_t)((160 * 1024) / (lds + 1024));
    uint32_t blocks = (uint32_t)device_info().cus * (per_cu < 1 ? 1 : (per_cu > 2 ? 2 : per_cu));
    const uint32_t need = cdiv(n_tiles, FF_WAVES);
    return blocks > need ? need : blocks;
}

template <int WIDTH>
static int launch_backward_backward(const void* grad, const void* inputs, const void* weights, const void* fwd, const void* u, uint32_t B,
                                    uint32_t in_dim, uint32_t num_layers, uint32_t act, void* grad_grad, void* grad_weights2, void* grad_inputs2,
                                    void* workspace, hipStream_t st) {
    constexpr int NIB = Shape<WIDTH>::NIB, NKB = Shape<WIDTH>::NKB;
    const bool slope = act_has_slope(act);
    const uint32_t n_tiles = B / FF_TILE, in_jb = (in_dim + 31) / 32;
    const bool need_dx = slope && grad_inputs2, need_w = grad_weights2 != nullptr;
    const bool need_s = slope && (need_dx || need_w);
    const bool need_d = need_w || need_s;
    const bool need_tangent = grad_grad || need_w || need_s;
    // every limit is checked before the first launch
    uint32_t frags_fwd = NIB * (in_dim / 16), frags_bwd = NIB * NKB;
    if (frags_fwd < (uint32_t)(NIB * NKB)) frags_fwd = NIB * NKB;
    if (need_dx && frags_bwd < in_jb * NKB) frags_bwd = in_jb * NKB;
    const size_t lds_fwd = (size_t)frags_fwd * 1024, lds_bwd = (size_t)frags_bwd * 1024, lds_d = (size_t)NIB * NKB * 1024;
    NGP_REQUIRE(lds_fwd <= 152 * 1024 && lds_bwd <= 152 * 1024, NGP_ERR_INVALID,
                "ffmlp_backward_backward: one %u x %u layer (%zu B) exceeds the LDS of a CU", (unsigned)WIDTH, in_dim,
                lds_fwd > lds_bwd ? lds_fwd : lds_bwd);
    const SecondWorkspace ws = second_workspace(B, in_dim, WIDTH, num_layers, act);
    unsigned char* base = static_cast<unsigned char*>(workspace);
    half_t* d_buf = reinterpret_cast<half_t*>(base + ws.d);
    half_t* p_buf = reinterpret_cast<half_t*>(base + ws.p);
    half_t* q_buf = reinterpret_cast<half_t*>(base + ws.q);
    half_t* s_buf = reinterpret_cast<half_t*>(base + ws.s);
    float* slabs = reinterpret_cast<float*>(base + ws.slabs);
    int rc;

    if (grad_inputs2 && !slope) {  // the first backward is linear in the inputs' direction: exactly zero
        hipError_t e = ::ngp::memset_async(grad_inputs2, 0, (size_t)B * in_dim * sizeof(half_t), st);
        NGP_REQUIRE(e == hipSuccess, NGP_ERR_LAUNCH, "ffmlp_backward_backward: hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    if (need_d) {  // d_l of the first backward, recomputed
        const void* dk = act == ACT_RELU ? reinterpret_cast<const void*>(k_ffmlp_dgrad_layered<WIDTH, true>)
                                         : reinterpret_cast<const void*>(k_ffmlp_dgrad_layered<WIDTH, false>);
        if ((rc = raise_lds(dk, lds_d, "ffmlp_backward_backward"))) return rc;
        const uint32_t blocks = layered_blocks(lds_d, n_tiles);
        if (act == ACT_RELU)
            NGP_LAUNCH((k_ffmlp_dgrad_layered<WIDTH, true>), dim3(blocks), dim3(FF_THREADS), lds_d, st, (const half_t*)grad, (const half_t*)weights,
                               (const half_t*)fwd, d_buf, n_tiles, in_dim, num_layers, act, false, (half_t*)nullptr, false);
        else
            NGP_LAUNCH((k_ffmlp_dgrad_layered<WIDTH, false>), dim3(blocks), dim3(FF_THREADS), lds_d, st, (const half_t*)grad, (const half_t*)weights,
                               (const half_t*)fwd, d_buf, n_tiles, in_dim, num_layers, act, false, (half_t*)nullptr, false);
        if ((rc = check_launch("ffmlp_backward_backward(dgrad)"))) return rc;
    }
    if (need_tangent) {
        auto kern = k_ffmlp_tangent_layered<WIDTH>;
        if ((rc = raise_lds(reinterpret_cast<const void*>(kern), lds_fwd, "ffmlp_backward_backward"))) return rc;
        NGP_LAUNCH(kern, dim3(layered_blocks(lds_fwd, n_tiles)), dim3(FF_THREADS), lds_fwd, st, (const half_t*)u, (const half_t*)weights,
                           (const half_t*)fwd, p_buf, need_s ? q_buf : (half_t*)nullptr, (half_t*)grad_grad, n_tiles, in_dim, num_layers, act);
        if ((rc = check_launch("ffmlp_backward_backward(tangent)"))) return rc;
    }
    if (need_s) {
        auto kern = k_ffmlp_dgrad2_layered<WIDTH>;
        if ((rc = raise_lds(reinterpret_cast<const void*>(kern), lds_bwd, "ffmlp_backward_backward"))) return rc;
        NGP_LAUNCH(kern, dim3(layered_blocks(lds_bwd, n_tiles)), dim3(FF_THREADS), lds_bwd, st, (const half_t*)grad, (const half_t*)weights,
                           (const half_t*)fwd, (const half_t*)d_buf, (const half_t*)q_buf, s_buf, n_tiles, in_dim, num_layers, act,
                           need_dx ? (half_t*)grad_inputs2 : (half_t*)nullptr);
        if ((rc = check_launch("ffmlp_backward_backward(dgrad2)"))) return rc;
    }
    if (!need_w) return NGP_OK;

    // weight terms: the contraction of k_ffmlp_wgrad twice -- explicit (u, p, d, grad) and implicit (inputs, h, s, no output-layer job) --
    // into two sets of fp32 slabs, one fixed-order reduction over both, one rounding
    const uint32_t n_params = ff_param_count(in_dim, WIDTH, num_layers);
    const uint32_t jobs_out = wgrad_jobs_of(1, NIB);
    const uint32_t jobs = wgrad_jobs_of(NIB, in_jb) + (num_layers - 1) * wgrad_jobs_of(NIB, NIB) + jobs_out;
    uint32_t chunks = cdiv((uint32_t)device_info().cus * 4u, jobs);  // ~4 workgroups per CU in flight
    if (chunks > WG_MAX_CHUNKS) chunks = WG_MAX_CHUNKS;
    const uint32_t by_tiles = cdiv(n_tiles, 2 * FF_WAVES);            // at least two rounds of tiles per wave
    if (chunks > by_tiles) chunks = by_tiles;
    if (chunks < 1) chunks = 1;
    const uint32_t tiles_per_chunk = cdiv(n_tiles, chunks);
    chunks = cdiv(n_tiles, tiles_per_chunk);
    NGP_LAUNCH(k_ffmlp_wgrad<WIDTH>, dim3(chunks, jobs), dim3(FF_THREADS), 0, st, (const half_t*)grad, (const half_t*)u, (const half_t*)p_buf,
                       (const half_t*)d_buf, n_tiles, in_dim, num_layers, false, tiles_per_chunk, slabs, (half_t*)nullptr);
    if ((rc = check_launch("ffmlp_backward_backward(wgrad, explicit)"))) return rc;
    uint32_t n_slabs = chunks;
    if (slope) {
        float* implicit = slabs + (size_t)chunks * n_params;
        // (the implicit terms have no output-layer part: that stretch of their slabs must read as zero in the reduction)
        hipError_t e = ::ngp::memset_async(implicit, 0, (size_t)chunks * n_params * sizeof(float), st);
        NGP_REQUIRE(e == hipSuccess, NGP_ERR_LAUNCH, "ffmlp_backward_backward: hipMemsetAsync failed: %s", hipGetErrorString(e));
        NGP_LAUNCH(k_ffmlp_wgrad<WIDTH>, dim3(chunks, jobs - jobs_out), dim3(FF_THREADS), 0, st, (const half_t*)nullptr, (const half_t*)inputs,
                           (const half_t*)fwd, (const half_t*)s_buf, n_tiles, in_dim, num_layers, false, tiles_per_chunk, implicit, (half_t*)nullptr);
        if ((rc = check_launch("ffmlp_backward_backward(wgrad, implicit)"))) return rc;
        n_slabs = 2 * chunks;
    }
    return reduce_slabs(slabs, n_slabs, n_params, grad_weights2, st, "ffmlp_backward_backward(reduce)");
}

}  // namespace ngp

extern "C" size_t ngp_ffmlp_backward_backward_workspace_bytes(uint32_t B, uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers,
                                                              uint32_t activation) {
    if (B == 0) return 0;
    return second_workspace(B, input_dim, hidden_dim, num_layers, activation).total;
}

extern "C" int ngp_ffmlp_backward_backward(const void* grad, const void* inputs, const void* weights, const void* forward_buffer, const void* u,
                                           uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                                           uint32_t activation, void* grad_grad, void* grad_weights2, void* grad_inputs2, void* workspace,
                                           size_t workspace_bytes, ngp_stream_t stream) {
    int rc = check_ff_args("ffmlp_backward_backward", B, input_dim, output_dim, hidden_dim, num_layers);
    if (rc) return rc;
    NGP_REQUIRE(activation <= ACT_NONE, NGP_ERR_INVALID, "ffmlp_backward_backward: unknown activation %u", activation);
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && inputs && weights && forward_buffer && u, NGP_ERR_INVALID, "ffmlp_backward_backward: NULL tensor");
    const size_t need = ngp_ffmlp_backward_backward_workspace_bytes(B, input_dim, hidden_dim, num_layers, activation);
    NGP_REQUIRE(workspace && workspace_bytes >= need, NGP_ERR_INVALID, "ffmlp_backward_backward: needs a workspace of %zu bytes (got %zu)", need,
                workspace ? workspace_bytes : (size_t)0);
    NGP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, NGP_ERR_INVALID, "ffmlp_backward_backward: the workspace must be 256-byte aligned");
    if (!grad_grad && !grad_weights2 && !grad_inputs2) return NGP_OK;
    hipStream_t st = as_stream(stream);
#define FF_SECOND(W) launch_backward_backward<W>(grad, inputs, weights, forward_buffer, u, B, input_dim, num_layers, activation, grad_grad, grad_weights2, grad_inputs2, workspace, st)
    FF_WIDTHS(FF_SECOND)
#undef FF_SECOND
}
