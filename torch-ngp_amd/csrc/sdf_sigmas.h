// NeuS's section opacity as the density that reproduces it (include/ngp_hip.h, ngp_sdf_sigmas_forward): the row arithmetic,
// the three kernel bodies and their launch, templated on the floating type -- float for sdf_sigmas.hip, double for the fp64 twins in fp64.hip.
// One lane per row, streaming: no LDS beyond the cross-wave partials of grad_inv_s, no private arrays.
//   c = dirs . normals,  ic = -(relu(0.5 - 0.5 c) (1 - cos_anneal) + relu(-c) cos_anneal),  h = 0.5 ic d0,  u-+ = inv_s (sdf -+ h)
//   x = log(sigmoid(u-) + eps) + softplus(-u+),   sigma = min(x, X_MAX) / d0   (0 for d0 == 0)
// x is -log(1 - alpha) of NeuS's alpha = (prev - next + eps) / (prev + eps) without the prev - next and the 1 - alpha cancellations.
#pragma once
#include "common.h"
#include <math.h>

namespace ngp {

constexpr int SDF_THREADS = 256, SDF_WAVES = SDF_THREADS / WAVE;
constexpr uint32_t SDF_MAX_ROWS = 1u << 31;   // block index * 256 + lane stays inside 32 bits
constexpr double SDF_EPS = 1e-5, SDF_X_MAX = 15.0;   // NeuS's epsilon; the bound of activation.trunc_exp

__device__ __forceinline__ float sdf_exp(float v) { return expf(v); }
__device__ __forceinline__ double sdf_exp(double v) { return exp(v); }
__device__ __forceinline__ float sdf_log(float v) { return logf(v); }
__device__ __forceinline__ double sdf_log(double v) { return log(v); }
__device__ __forceinline__ float sdf_log1p(float v) { return log1pf(v); }
__device__ __forceinline__ double sdf_log1p(double v) { return log1p(v); }
__device__ __forceinline__ float sdf_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double sdf_abs(double v) { return fabs(v); }

// the logistic function without overflow: e = exp(-|u|) <= 1
template <typename F>
__device__ __forceinline__ F sdf_sigmoid(F u) {
    const F e = sdf_exp(-sdf_abs(u));
    return (u >= F(0) ? F(1) : e) / (F(1) + e);
}
// log(1 + exp(z)) = max(z, 0) + log1p(exp(-|z|))
template <typename F>
__device__ __forceinline__ F sdf_softplus(F z) { return (z > F(0) ? z : F(0)) + sdf_log1p(sdf_exp(-sdf_abs(z))); }

// what forward and backward share of a row
template <typename F>
struct SdfRow {
    F c, h, um, up, P, x;
};
template <typename F>
__device__ __forceinline__ SdfRow<F> sdf_row(F sdf, const F* n, const F* d, F d0, F inv_s, F ca) {
    SdfRow<F> r;
    r.c = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
    const F a = F(0.5) - F(0.5) * r.c, b = -r.c;
    const F ic = -((a > F(0) ? a : F(0)) * (F(1) - ca) + (b > F(0) ? b : F(0)) * ca);
    r.h = (F(0.5) * ic) * d0;
    r.um = inv_s * (sdf - r.h);
    r.up = inv_s * (sdf + r.h);
    r.P = sdf_sigmoid(r.um);
    r.x = sdf_log(r.P + F(SDF_EPS)) + sdf_softplus(-r.up);
    return r;
}

// The three kernel bodies; the __global__ functions that carry them are defined per unit (SDF_SIGMAS_KERNELS below), so that the double
// instances bear the k_f64_ names of fp64.hip's kernels.
template <typename F>
__device__ __forceinline__ void sdf_sigmas_fwd_body(const F* __restrict__ sdf, const F* __restrict__ normals, const F* __restrict__ dirs,
                                                    const F* __restrict__ deltas, const F* __restrict__ inv_s, uint32_t M, F ca, F* __restrict__ sigmas) {
    const uint32_t i = blockIdx.x * SDF_THREADS + threadIdx.x;
    if (i >= M) return;
    typedef F pair_t __attribute__((ext_vector_type(2)));
    const pair_t dl = reinterpret_cast<const pair_t*>(deltas)[i];   // one 8-byte (fp64: 16-byte) load; only d0 is used
    const F d0 = dl.x;
    F out = F(0);
    if (d0 > F(0)) {
        const size_t o = (size_t)i * 3u;
        const F n[3] = {normals[o], normals[o + 1u], normals[o + 2u]}, d[3] = {dirs[o], dirs[o + 1u], dirs[o + 2u]};
        const SdfRow<F> r = sdf_row<F>(sdf[i], n, d, d0, inv_s[0], ca);
        out = (r.x < F(SDF_X_MAX) ? r.x : F(SDF_X_MAX)) / d0;
    }
    sigmas[i] = out;
}

// grad_sdf / grad_normals / grad_dirs (optional) of every row -- zeros for padding rows (d0 == 0) and capped rows (x >= X_MAX: the derivative of
// min) -- and the workgroup's share of grad_inv_s, summed in double in a fixed order: xor tree per wave, the waves in order.
template <typename F>
__device__ __forceinline__ void sdf_sigmas_bwd_body(const F* __restrict__ grad_sigmas, const F* __restrict__ sdf, const F* __restrict__ normals,
                                                    const F* __restrict__ dirs, const F* __restrict__ deltas, const F* __restrict__ inv_s, uint32_t M,
                                                    F ca, F* __restrict__ grad_sdf, F* __restrict__ grad_normals, F* __restrict__ grad_dirs,
                                                    double* __restrict__ partials) {
    __shared__ double wave_part[SDF_WAVES];
    const uint32_t i = blockIdx.x * SDF_THREADS + threadIdx.x;
    double term = 0.0;
    if (i < M) {
        typedef F pair_t __attribute__((ext_vector_type(2)));
        const pair_t dl = reinterpret_cast<const pair_t*>(deltas)[i];
        const F d0 = dl.x;
        const size_t o = (size_t)i * 3u;
        F gs = F(0), gn[3] = {F(0), F(0), F(0)}, gd[3] = {F(0), F(0), F(0)};
        if (d0 > F(0)) {
            const F n[3] = {normals[o], normals[o + 1u], normals[o + 2u]}, d[3] = {dirs[o], dirs[o + 1u], dirs[o + 2u]};
            const F s = sdf[i], k = inv_s[0];
            const SdfRow<F> r = sdf_row<F>(s, n, d, d0, k, ca);
            if (r.x < F(SDF_X_MAX)) {
                const F gx = grad_sigmas[i] / d0;
                const F A = r.P * sdf_sigmoid(-r.um) / (r.P + F(SDF_EPS)), B = sdf_sigmoid(-r.up);   // 1 - P as sigmoid(-u-): no cancellation
                gs = gx * (k * (A - B));
                const F dh_dc = (F(0.5) * d0) * ((r.c < F(1) ? F(0.5) * (F(1) - ca) : F(0)) + (r.c < F(0) ? ca : F(0)));
                const F gc = (gx * (-k * (A + B))) * dh_dc;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    gn[j] = gc * d[j];
                    gd[j] = gc * n[j];
                }
                term = (double)(gx * (A * (s - r.h) - B * (s + r.h)));
            }
        }
        grad_sdf[i] = gs;
#pragma unroll
        for (int j = 0; j < 3; j++) grad_normals[o + j] = gn[j];
        if (grad_dirs) {
#pragma unroll
            for (int j = 0; j < 3; j++) grad_dirs[o + j] = gd[j];
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) term += __shfl_xor(term, w, 64);
    if ((threadIdx.x & 63u) == 0u) wave_part[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0u) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < SDF_WAVES; w++) v += wave_part[w];
        partials[blockIdx.x] = v;
    }
}

// the last pass, one workgroup: thread t adds partials[t], partials[t + 256], ... in index order, then the same wave / workgroup order as
// above; one rounding to F at the end
template <typename F>
__device__ __forceinline__ void sdf_sigmas_inv_s_body(const double* __restrict__ partials, uint32_t n_partials, F* __restrict__ grad_inv_s) {
    __shared__ double wave_part[SDF_WAVES];
    double term = 0.0;
    for (uint32_t p = threadIdx.x; p < n_partials; p += SDF_THREADS) term += partials[p];
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) term += __shfl_xor(term, w, 64);
    if ((threadIdx.x & 63u) == 0u) wave_part[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0u) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < SDF_WAVES; w++) v += wave_part[w];
        grad_inv_s[0] = (F)v;
    }
}

// the unit's kernels: SDF_SIGMAS_KERNELS(float, k_sdf_sigmas) defines k_sdf_sigmas_fwd / _bwd / _inv_s
#define SDF_SIGMAS_KERNELS(F, PREFIX)                                                                                                             \
    __global__ __launch_bounds__(SDF_THREADS) void PREFIX##_fwd(const F* sdf, const F* normals, const F* dirs, const F* deltas, const F* inv_s, \
                                                                uint32_t M, F ca, F* sigmas) {                                                  \
        sdf_sigmas_fwd_body<F>(sdf, normals, dirs, deltas, inv_s, M, ca, sigmas);                                                               \
    }                                                                                                                                           \
    __global__ __launch_bounds__(SDF_THREADS) void PREFIX##_bwd(const F* grad_sigmas, const F* sdf, const F* normals, const F* dirs,            \
                                                                const F* deltas, const F* inv_s, uint32_t M, F ca, F* grad_sdf,                 \
                                                                F* grad_normals, F* grad_dirs, double* partials) {                              \
        sdf_sigmas_bwd_body<F>(grad_sigmas, sdf, normals, dirs, deltas, inv_s, M, ca, grad_sdf, grad_normals, grad_dirs, partials);             \
    }                                                                                                                                           \
    __global__ __launch_bounds__(SDF_THREADS) void PREFIX##_inv_s(const double* partials, uint32_t n_partials, F* grad_inv_s) {                 \
        sdf_sigmas_inv_s_body<F>(partials, n_partials, grad_inv_s);                                                                             \
    }
template <typename F>
struct SdfKernels {
    void (*fwd)(const F*, const F*, const F*, const F*, const F*, uint32_t, F, F*);
    void (*bwd)(const F*, const F*, const F*, const F*, const F*, const F*, uint32_t, F, F*, F*, F*, double*);
    void (*inv_s)(const double*, uint32_t, F*);
};

// ---- host side: one statement of the validation and the launches for both types ----
inline uint32_t sdf_sigmas_blocks(uint32_t M) { return M / SDF_THREADS + (M % SDF_THREADS ? 1u : 0u); }   // (no wrap for M near 2^32)
inline size_t sdf_sigmas_workspace_bytes(uint32_t M) { return (size_t)sdf_sigmas_blocks(M) * sizeof(double); }

template <typename F>
int sdf_sigmas_forward(const char* fn, const SdfKernels<F>& k, const F* sdf, const F* normals, const F* dirs, const F* deltas, const F* inv_s, uint32_t M, float cos_anneal,
                       F* sigmas, hipStream_t st) {
    NGP_REQUIRE(cos_anneal >= 0.0f && cos_anneal <= 1.0f, NGP_ERR_INVALID, "%s: cos_anneal must be in [0, 1] (got %g)", fn, (double)cos_anneal);
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(M <= SDF_MAX_ROWS, NGP_ERR_INVALID, "%s: M = %u is above 2^31 rows", fn, M);
    NGP_REQUIRE(sdf && normals && dirs && deltas && inv_s && sigmas, NGP_ERR_INVALID, "%s: NULL tensor", fn);
    (void)launch("k_sdf_sigmas_fwd", k.fwd, dim3(sdf_sigmas_blocks(M)), dim3(SDF_THREADS), 0, st, sdf, normals, dirs, deltas, inv_s, M, (F)cos_anneal, sigmas);
    return check_launch(fn);
}

template <typename F>
int sdf_sigmas_backward(const char* fn, const SdfKernels<F>& k, const F* grad_sigmas, const F* sdf, const F* normals, const F* dirs, const F* deltas, const F* inv_s, uint32_t M,
                        float cos_anneal, F* grad_sdf, F* grad_normals, F* grad_dirs, F* grad_inv_s, void* workspace, size_t workspace_bytes,
                        hipStream_t st) {
    NGP_REQUIRE(cos_anneal >= 0.0f && cos_anneal <= 1.0f, NGP_ERR_INVALID, "%s: cos_anneal must be in [0, 1] (got %g)", fn, (double)cos_anneal);
    if (M == 0) return NGP_OK;
    NGP_REQUIRE(M <= SDF_MAX_ROWS, NGP_ERR_INVALID, "%s: M = %u is above 2^31 rows", fn, M);
    NGP_REQUIRE(grad_sigmas && sdf && normals && dirs && deltas && inv_s && grad_sdf && grad_normals && grad_inv_s, NGP_ERR_INVALID,
                "%s: NULL tensor (only grad_dirs may be NULL)", fn);
    const size_t need = sdf_sigmas_workspace_bytes(M);
    NGP_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0u, NGP_ERR_INVALID,
                "%s: workspace of %zu bytes is smaller than ngp_sdf_sigmas_workspace_bytes(%u) = %zu, NULL or not 8-byte aligned", fn, workspace_bytes, M,
                need);
    const uint32_t blocks = sdf_sigmas_blocks(M);
    double* partials = static_cast<double*>(workspace);
    (void)launch("k_sdf_sigmas_bwd", k.bwd, dim3(blocks), dim3(SDF_THREADS), 0, st, grad_sigmas, sdf, normals, dirs, deltas, inv_s, M, (F)cos_anneal, grad_sdf,
                 grad_normals, grad_dirs, partials);
    (void)launch("k_sdf_sigmas_inv_s", k.inv_s, dim3(1), dim3(SDF_THREADS), 0, st, (const double*)partials, blocks, grad_inv_s);
    return check_launch(fn);
}

}  // namespace ngp
