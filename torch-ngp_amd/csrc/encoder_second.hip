// Second-order backward of the frequency and spherical-harmonics encoders for gfx950 (MI355X), and the frequency encoder in fp64: the
// backward of each first backward, so that a loss on d enc / d x (eikonal / normal losses: torch.autograd.grad(sdf, x, create_graph=True))
// reaches the upstream gradient and the inputs.  With u = dL/dgx of the first backward's result gx:
//
//   frequency (freqencoder.hip: gx_d = g_d + sum_f 2^f (g_sin[f,d] o_cos[f,d] - g_cos[f,d] o_sin[f,d]) from the stored outputs o):
//     dL/dg [B,C]:  identity block u_d,  sin slot 2^f u_d o_cos[f,d],  cos slot -2^f u_d o_sin[f,d]
//     dL/dx [B,D]:  -u_d sum_f 4^f (g_sin[f,d] o_sin[f,d] + g_cos[f,d] o_cos[f,d])
//   SH (shencoder.hip: gx_d = sum_i g_i dy_dx[b,d,i]):
//     dL/dg [B,N]:  sum_d u_d dy_dx[b,d,i]                        from the stored dy_dx
//     dL/dx [B,3]:  sum_i g_i sum_d u_d d2Y_i/dx_d dx_e           the Hessians of the basis polynomials (sh_hess.inc, tools/gen_sh.py)
//
// All four are pure streams without atomics, every sum in a fixed order (deterministic), every output overwritten.
//   * k_freq_bwd_bwd: a block owns P consecutive points, i.e. one contiguous span of P*C elements of g, o and dL/dg.  One lane per
//     element reads g and o once (coalesced), writes dL/dg (the partner slot o[t +- D] is a shifted read of the same span: L1) and
//     leaves g*o in LDS; then one lane per (point, d) sums its row of products -- the read with a stride of C floats -- out of LDS
//     (row stride C | 1: odd, so the lanes of a point's neighbours fall on different banks).  4 (3C + 2D) bytes per point.
//     Rows too wide for the tile (C > 4096 floats / 2048 doubles: D >= 33 at any degree whose 4^f is finite) take k_freq_bwd_bwd_wide,
//     one lane per element / per (point, d) straight from global memory: with such a D the lanes of a wave read consecutive d.
//   * k_sh_bwd_bwd_g: one lane per element of dL/dg; the three dy_dx reads of a wave are runs of N consecutive floats which together
//     cover the wave's span of dy_dx exactly once.
//   * k_sh_bwd_bwd_x: one lane per point.  The wave's 64 rows of g are one contiguous span: staged through LDS (coalesced read), then each
//     lane reads its row (stride N | 1 floats: conflict-free) while it evaluates the Hessian polynomials; each expression is consumed as
//     it is produced (acc_e += g_i u_d H_i[d,e]), so no table lives in registers.
// fp64 frequency forward / first backward: freqencoder.hip's two kernels on double, cos as sin(. + pi/2) in double.
#include "common.h"
#include "sh_hess.inc"
#include "sh_hess64.inc"
#include <math.h>

namespace ngp {

constexpr int ES_THREADS = 256;
constexpr int ES_TILE_BYTES = 16384;  // k_freq_bwd_bwd's products

__device__ __forceinline__ float es_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double es_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float es_scalbn(float a, int n) { return scalbnf(a, n); }
__device__ __forceinline__ double es_scalbn(double a, int n) { return scalbn(a, n); }

// ------------------------------------------------------------------------------------------------
// frequency encoder, fp64 forward and first backward (freqencoder.hip on double)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_THREADS) void k_f64_freq_forward(const double* __restrict__ inputs, uint32_t B, uint32_t D, uint32_t C,
                                                                 double* __restrict__ outputs) {
    const uint64_t total = (uint64_t)B * C;
    for (uint64_t t = (uint64_t)blockIdx.x * ES_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * ES_THREADS) {
        const uint32_t b = (uint32_t)(t / C), c = (uint32_t)(t - (uint64_t)b * C);
        const double* x = inputs + (size_t)b * D;
        double v;
        if (c < D) {
            v = x[c];
        } else {
            const uint32_t col = c / D - 1u, d = c % D;
            const double phase = (col & 1u) ? 1.5707963267948966 : 0.0;
            v = sin(scalbn(x[d], (int)(col >> 1)) + phase);
        }
        outputs[t] = v;
    }
}

__global__ __launch_bounds__(ES_THREADS) void k_f64_freq_backward(const double* __restrict__ grad, const double* __restrict__ outputs, uint32_t B,
                                                                  uint32_t D, uint32_t deg, uint32_t C, double* __restrict__ grad_inputs) {
    const uint64_t total = (uint64_t)B * D;
    for (uint64_t t = (uint64_t)blockIdx.x * ES_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * ES_THREADS) {
        const uint32_t b = (uint32_t)(t / D), d = (uint32_t)(t - (uint64_t)b * D);
        const double* g = grad + (size_t)b * C;
        const double* o = outputs + (size_t)b * C;
        double r = g[d];
        for (uint32_t f = 0; f < deg; f++) {
            const uint32_t s = D + 2u * f * D + d, c = s + D;  // sin and cos slots of frequency f
            r += scalbn(1.0, (int)f) * (g[s] * o[c] - g[c] * o[s]);
        }
        grad_inputs[t] = r;
    }
}

// ------------------------------------------------------------------------------------------------
// frequency encoder, second order
// ------------------------------------------------------------------------------------------------
// element c of a point's dL/dg row; o_row: the point's stored outputs
template <typename T>
__device__ __forceinline__ T freq_grad_grad(const T* __restrict__ u_row, const T* __restrict__ o_row, uint32_t c, uint32_t D) {
    if (c < D) return u_row[c];
    const uint32_t col = c / D - 1u, d = c - (col + 1u) * D;
    const T su = es_scalbn(u_row[d], (int)(col >> 1));  // exact: a power-of-two scale
    return (col & 1u) ? -(su * o_row[c - D]) : su * o_row[c + D];
}

// dL/dx of one (point, d) from the products p[c] = g[c] o[c] of its row
template <typename T>
__device__ __forceinline__ T freq_grad_inputs2(const T* p, T u, uint32_t d, uint32_t D, uint32_t deg) {
    T acc = (T)0;
    for (uint32_t f = 0; f < deg; f++) {
        const uint32_t s = D + 2u * f * D + d;
        acc = es_fma(es_scalbn((T)1, 2 * (int)f), p[s] + p[s + D], acc);
    }
    return -(u * acc);
}

template <typename T>
__global__ __launch_bounds__(ES_THREADS) void k_freq_bwd_bwd(const T* __restrict__ grad, const T* __restrict__ outputs, const T* __restrict__ u,
                                                             uint32_t B, uint32_t D, uint32_t deg, uint32_t C, uint32_t P, uint32_t CP,
                                                             T* __restrict__ grad_grad, T* __restrict__ grad_inputs2) {
    constexpr uint32_t TILE = ES_TILE_BYTES / sizeof(T);
    __shared__ T prod[TILE];  // [P][CP], host: P * CP <= TILE
    const uint64_t b0 = (uint64_t)blockIdx.x * P;
    const uint32_t n_pts = (uint32_t)min((uint64_t)P, (uint64_t)B - b0);
    const T* __restrict__ g = grad + b0 * C;
    const T* __restrict__ o = outputs + b0 * C;
    const T* __restrict__ ub = u + b0 * D;
    const uint32_t n_el = n_pts * C;
    for (uint32_t i = threadIdx.x; i < n_el; i += ES_THREADS) {
        const uint32_t pt = i / C, c = i - pt * C;
        if (grad_grad) grad_grad[b0 * C + i] = freq_grad_grad<T>(ub + (size_t)pt * D, o + (size_t)pt * C, c, D);
        if (grad_inputs2) {
            NGP_BOUNDS(pt * CP + c < TILE);
            prod[pt * CP + c] = g[i] * o[i];
        }
    }
    if (!grad_inputs2) return;  // (block-uniform)
    __syncthreads();
    const uint32_t n_out = n_pts * D;
    for (uint32_t j = threadIdx.x; j < n_out; j += ES_THREADS) {
        const uint32_t pt = j / D, d = j - pt * D;
        grad_inputs2[b0 * D + j] = freq_grad_inputs2<T>(prod + pt * CP, ub[j], d, D, deg);
    }
}

// rows wider than the LDS tile: straight from global memory
template <typename T>
__global__ __launch_bounds__(ES_THREADS) void k_freq_bwd_bwd_wide(const T* __restrict__ grad, const T* __restrict__ outputs, const T* __restrict__ u,
                                                                  uint32_t B, uint32_t D, uint32_t deg, uint32_t C, T* __restrict__ grad_grad,
                                                                  T* __restrict__ grad_inputs2) {
    const uint64_t first = (uint64_t)blockIdx.x * ES_THREADS + threadIdx.x, step = (uint64_t)gridDim.x * ES_THREADS;
    if (grad_grad) {
        const uint64_t total = (uint64_t)B * C;
        for (uint64_t t = first; t < total; t += step) {
            const uint32_t b = (uint32_t)(t / C), c = (uint32_t)(t - (uint64_t)b * C);
            grad_grad[t] = freq_grad_grad<T>(u + (size_t)b * D, outputs + (size_t)b * C, c, D);
        }
    }
    if (grad_inputs2) {
        const uint64_t total = (uint64_t)B * D;
        for (uint64_t t = first; t < total; t += step) {
            const uint32_t b = (uint32_t)(t / D), d = (uint32_t)(t - (uint64_t)b * D);
            const T* g = grad + (size_t)b * C;
            const T* o = outputs + (size_t)b * C;
            T acc = (T)0;
            for (uint32_t f = 0; f < deg; f++) {
                const uint32_t s = D + 2u * f * D + d;
                acc = es_fma(es_scalbn((T)1, 2 * (int)f), g[s] * o[s] + g[s + D] * o[s + D], acc);  // as freq_grad_inputs2
            }
            grad_inputs2[t] = -(u[t] * acc);
        }
    }
}

template <typename T>
static int launch_freq_bwd_bwd(const void* grad, const void* outputs, const void* u, uint32_t B, uint32_t D, uint32_t deg, uint32_t C, void* grad_grad,
                               void* grad_inputs2, hipStream_t st) {
    constexpr uint32_t TILE = ES_TILE_BYTES / sizeof(T);
    const uint32_t CP = C | 1u;
    if (CP <= TILE) {
        const uint32_t P = min(TILE / CP, (uint32_t)ES_THREADS);
        NGP_LAUNCH((k_freq_bwd_bwd<T>), dim3((uint32_t)cdiv64(B, P)), dim3(ES_THREADS), 0, st, (const T*)grad, (const T*)outputs, (const T*)u, B, D, deg,
                           C, P, CP, (T*)grad_grad, (T*)grad_inputs2);
    } else {
        uint64_t blocks = cdiv64((uint64_t)B * C, ES_THREADS);
        if (blocks > 65536u) blocks = 65536u;
        NGP_LAUNCH((k_freq_bwd_bwd_wide<T>), dim3((uint32_t)blocks), dim3(ES_THREADS), 0, st, (const T*)grad, (const T*)outputs, (const T*)u, B, D,
                           deg, C, (T*)grad_grad, (T*)grad_inputs2);
    }
    return check_launch("freq_encode_backward_backward");
}

// ------------------------------------------------------------------------------------------------
// SH encoder, second order
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(ES_THREADS) void k_sh_bwd_bwd_g(const T* __restrict__ dy_dx, const T* __restrict__ u, uint32_t B, uint32_t N,
                                                             T* __restrict__ grad_grad) {
    const uint64_t total = (uint64_t)B * N;
    for (uint64_t t = (uint64_t)blockIdx.x * ES_THREADS + threadIdx.x; t < total; t += (uint64_t)gridDim.x * ES_THREADS) {
        const uint32_t b = (uint32_t)(t / N), i = (uint32_t)(t - (uint64_t)b * N);
        const T* dd = dy_dx + (size_t)b * 3 * N + i;
        const T* ub = u + (size_t)b * 3;
        T r = ub[0] * dd[0];
        r = es_fma(ub[1], dd[N], r);
        r = es_fma(ub[2], dd[2 * (size_t)N], r);
        grad_grad[t] = r;
    }
}

// the per-band Hessian macros of a precision (bands 0 and 1 have none: constant and linear polynomials)
#define NGP_SH_HESS_BANDS(P)                      \
    if constexpr (BANDS > 2) { P##_BAND_2_HESS; } \
    if constexpr (BANDS > 3) { P##_BAND_3_HESS; } \
    if constexpr (BANDS > 4) { P##_BAND_4_HESS; } \
    if constexpr (BANDS > 5) { P##_BAND_5_HESS; } \
    if constexpr (BANDS > 6) { P##_BAND_6_HESS; } \
    if constexpr (BANDS > 7) { P##_BAND_7_HESS; }

// one lane per point; WAVES waves per block (the g rows of a wave: 64 * (N | 1) elements of LDS)
template <typename T, int BANDS, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_sh_bwd_bwd_x(const T* __restrict__ grad, const T* __restrict__ inputs, const T* __restrict__ uin,
                                                             uint32_t B, T* __restrict__ grad_inputs2) {
    constexpr int N = BANDS * BANDS, NP = N | 1;
    __shared__ T stage[WAVES][64 * NP];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t wave_base = ((uint64_t)blockIdx.x * WAVES + wid) * 64;  // first point of this wave
    const uint64_t b = wave_base + lane;
    const bool valid = b < B;
    const uint32_t n_valid = wave_base < B ? (uint32_t)min((uint64_t)64, (uint64_t)B - wave_base) : 0u;
    T* row = stage[wid];
    {
        const T* src = grad + wave_base * N;
        const uint32_t total = n_valid * N;
        for (uint32_t i = lane; i < total; i += 64) row[(i / N) * NP + (i % N)] = src[i];
        for (uint32_t i = total + lane; i < 64u * N; i += 64) row[(i / N) * NP + (i % N)] = (T)0;  // rows of lanes past the end
    }
    __syncthreads();  // (every wave of the block arrives: a wave past the end staged zeros)
    T x = (T)0, y = (T)0, z = (T)0, ux = (T)0, uy = (T)0, uz = (T)0;
    if (valid) {
        x = inputs[b * 3], y = inputs[b * 3 + 1], z = inputs[b * 3 + 2];
        ux = uin[b * 3], uy = uin[b * 3 + 1], uz = uin[b * 3 + 2];
    }
    const T* gr = row + lane * NP;
    T ax = (T)0, ay = (T)0, az = (T)0;
    // acc_e += g_i * (u . H_i[:, e]); a mixed derivative serves both of its columns
#define SH_HXX(i, v) { const T h_ = (v); ax = es_fma(gr[i] * ux, h_, ax); }
#define SH_HYY(i, v) { const T h_ = (v); ay = es_fma(gr[i] * uy, h_, ay); }
#define SH_HZZ(i, v) { const T h_ = (v); az = es_fma(gr[i] * uz, h_, az); }
#define SH_HXY(i, v) { const T h_ = (v); ax = es_fma(gr[i] * uy, h_, ax); ay = es_fma(gr[i] * ux, h_, ay); }
#define SH_HXZ(i, v) { const T h_ = (v); ax = es_fma(gr[i] * uz, h_, ax); az = es_fma(gr[i] * ux, h_, az); }
#define SH_HYZ(i, v) { const T h_ = (v); ay = es_fma(gr[i] * uz, h_, ay); az = es_fma(gr[i] * uy, h_, az); }
    if constexpr (sizeof(T) == 8) {
        NGP_SH_HESS_BANDS(SH64)
    } else {
        NGP_SH_HESS_BANDS(SH)
    }
#undef SH_HXX
#undef SH_HYY
#undef SH_HZZ
#undef SH_HXY
#undef SH_HXZ
#undef SH_HYZ
    if (valid) {
        grad_inputs2[b * 3] = ax;
        grad_inputs2[b * 3 + 1] = ay;
        grad_inputs2[b * 3 + 2] = az;
    }
}

template <typename T, int BANDS>
static int launch_sh_bwd_bwd_x(const void* grad, const void* inputs, const void* u, uint32_t B, void* grad_inputs2, hipStream_t st) {
    // 64 * (N | 1) elements of LDS per wave: at degree 8 66560 B = 65 KiB per block (4 x 16640 B in fp32, 2 x 33280 B in fp64) of the CU's
    // 160 KiB, i.e. two blocks per CU there
    constexpr int WAVES = sizeof(T) == 8 ? 2 : 4;
    NGP_LAUNCH((k_sh_bwd_bwd_x<T, BANDS, WAVES>), dim3((uint32_t)cdiv64(B, WAVES * 64)), dim3(WAVES * 64), 0, st, (const T*)grad, (const T*)inputs,
                       (const T*)u, B, (T*)grad_inputs2);
    return check_launch("sh_encode_backward_backward");
}

template <typename T>
static int launch_sh_bwd_bwd(const void* grad, const void* inputs, const void* dy_dx, const void* u, uint32_t B, uint32_t C, void* grad_grad,
                             void* grad_inputs2, hipStream_t st) {
    if (grad_grad) {
        uint64_t blocks = cdiv64((uint64_t)B * C * C, ES_THREADS);
        if (blocks > 65536u) blocks = 65536u;
        NGP_LAUNCH((k_sh_bwd_bwd_g<T>), dim3((uint32_t)blocks), dim3(ES_THREADS), 0, st, (const T*)dy_dx, (const T*)u, B, C * C, (T*)grad_grad);
        const int rc = check_launch("sh_encode_backward_backward");
        if (rc) return rc;
    }
    if (!grad_inputs2) return NGP_OK;
    switch (C) {
        case 1:
        case 2: {  // constant and linear polynomials have no Hessian: zeros, without reading g
            const hipError_t e = ::ngp::memset_async(grad_inputs2, 0, (size_t)B * 3 * sizeof(T), st);
            NGP_REQUIRE(e == hipSuccess, NGP_ERR_LAUNCH, "sh_encode_backward_backward: zero fill failed: %s", hipGetErrorString(e));
            return NGP_OK;
        }
        case 3: return launch_sh_bwd_bwd_x<T, 3>(grad, inputs, u, B, grad_inputs2, st);
        case 4: return launch_sh_bwd_bwd_x<T, 4>(grad, inputs, u, B, grad_inputs2, st);
        case 5: return launch_sh_bwd_bwd_x<T, 5>(grad, inputs, u, B, grad_inputs2, st);
        case 6: return launch_sh_bwd_bwd_x<T, 6>(grad, inputs, u, B, grad_inputs2, st);
        case 7: return launch_sh_bwd_bwd_x<T, 7>(grad, inputs, u, B, grad_inputs2, st);
        default: return launch_sh_bwd_bwd_x<T, 8>(grad, inputs, u, B, grad_inputs2, st);
    }
}

}  // namespace ngp

using namespace ngp;

static int check_freq(const char* fn, uint32_t D, uint32_t deg, uint32_t C) {  // (freqencoder.hip)
    NGP_REQUIRE(D >= 1, NGP_ERR_INVALID, "%s: input dim must be positive", fn);
    NGP_REQUIRE(C == D + 2u * D * deg, NGP_ERR_INVALID, "%s: output_dim must be input_dim + 2 * input_dim * degree (got %u for D=%u, degree=%u)",
                fn, C, D, deg);
    return NGP_OK;
}

extern "C" int ngp_freq_encode_forward_f64(const double* inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C, double* outputs,
                                           ngp_stream_t stream) {
    int rc = check_freq("freq_encode_forward_f64", D, deg, C);
    if (rc) return rc;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(inputs && outputs, NGP_ERR_INVALID, "freq_encode_forward_f64: NULL tensor");
    uint64_t blocks = cdiv64((uint64_t)B * C, ES_THREADS);
    if (blocks > 65536u) blocks = 65536u;
    NGP_LAUNCH(k_f64_freq_forward, dim3((uint32_t)blocks), dim3(ES_THREADS), 0, as_stream(stream), inputs, B, D, C, outputs);
    return check_launch("freq_encode_forward_f64");
}

extern "C" int ngp_freq_encode_backward_f64(const double* grad, const double* outputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                                            double* grad_inputs, ngp_stream_t stream) {
    int rc = check_freq("freq_encode_backward_f64", D, deg, C);
    if (rc) return rc;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && outputs && grad_inputs, NGP_ERR_INVALID, "freq_encode_backward_f64: NULL tensor");
    uint64_t blocks = cdiv64((uint64_t)B * D, ES_THREADS);
    if (blocks > 65536u) blocks = 65536u;
    NGP_LAUNCH(k_f64_freq_backward, dim3((uint32_t)blocks), dim3(ES_THREADS), 0, as_stream(stream), grad, outputs, B, D, deg, C, grad_inputs);
    return check_launch("freq_encode_backward_f64");
}

extern "C" int ngp_freq_encode_backward_backward(const void* grad, const void* outputs, const void* u, uint32_t B, uint32_t D, uint32_t deg,
                                                 uint32_t C, void* grad_grad, void* grad_inputs2, int dtype, ngp_stream_t stream) {
    const char* fn = "freq_encode_backward_backward";
    int rc = check_freq(fn, D, deg, C);
    if (rc) return rc;
    NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F64, NGP_ERR_INVALID, "%s: second order is provided for float32 and float64", fn);
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && outputs && u, NGP_ERR_INVALID, "%s: NULL tensor", fn);
    if (!grad_grad && !grad_inputs2) return NGP_OK;
    return dtype == NGP_F64 ? launch_freq_bwd_bwd<double>(grad, outputs, u, B, D, deg, C, grad_grad, grad_inputs2, as_stream(stream))
                            : launch_freq_bwd_bwd<float>(grad, outputs, u, B, D, deg, C, grad_grad, grad_inputs2, as_stream(stream));
}

extern "C" int ngp_sh_encode_backward_backward(const void* grad, const void* inputs, const void* dy_dx, const void* u, uint32_t B, uint32_t D,
                                               uint32_t C, void* grad_grad, void* grad_inputs2, int dtype, ngp_stream_t stream) {
    const char* fn = "sh_encode_backward_backward";
    NGP_REQUIRE(D == 3, NGP_ERR_INVALID, "%s: SH encoder only support input dim == 3 (got %u)", fn, D);
    NGP_REQUIRE(C >= 1 && C <= 8, NGP_ERR_INVALID, "%s: SH encoder only supports degree in [1, 8] (got %u)", fn, C);
    NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F64, NGP_ERR_INVALID, "%s: second order is provided for float32 and float64", fn);
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && inputs && dy_dx && u, NGP_ERR_INVALID, "%s: NULL tensor", fn);
    return dtype == NGP_F64 ? launch_sh_bwd_bwd<double>(grad, inputs, dy_dx, u, B, C, grad_grad, grad_inputs2, as_stream(stream))
                            : launch_sh_bwd_bwd<float>(grad, inputs, dy_dx, u, B, C, grad_grad, grad_inputs2, as_stream(stream));
}
