// The second-order backward's per-corner terms and its per-point kernel (the u-terms of grid_second.hip), in a header so that the ordered
// scatter (grid_ordered.hip) gets grad_grad / grad_inputs2 from a gather-only instantiation of the same kernel: the same bits as
// ngp_grid_encode_backward_backward.  Also record_coeff: what a sorted record (grid_records.h) contributes to its table entry, first and
// second order, for the run sums of fp64.hip and grid_ordered.hip.
#pragma once
#include "common.h"
#include "grid_index.h"
#include <math.h>

namespace ngp {

constexpr int GG_THREADS = 256;

template <typename T>
struct GGAcc {
    using type = float;  // fp16 and fp32 tables accumulate in fp32
};
template <>
struct GGAcc<double> {
    using type = double;
};

__device__ __forceinline__ float gg_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double gg_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

typedef uint32_t gg_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t gg_u32x4 __attribute__((ext_vector_type(4)));

// C consecutive values of a row (rows are C-aligned: one vector load of 4 / 8 / 16 bytes, or several 16-byte ones), converted to A
template <typename T, typename A, int C>
__device__ __forceinline__ void load_row(const T* __restrict__ p, A (&v)[C]) {
    constexpr int BYTES = C * (int)sizeof(T);
    T t[C];
    if constexpr (BYTES % 16 == 0) {
#pragma unroll
        for (int i = 0; i < BYTES / 16; i++) {
            const gg_u32x4 w = reinterpret_cast<const gg_u32x4*>(p)[i];
            __builtin_memcpy(reinterpret_cast<char*>(t) + 16 * i, &w, 16);
        }
    } else if constexpr (BYTES == 8) {
        const gg_u32x2 w = *reinterpret_cast<const gg_u32x2*>(p);
        __builtin_memcpy(t, &w, 8);
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) t[c] = p[c];
    }
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = (A)t[c];
}

// Corner k (bit d set: the upper vertex in dimension d): returns a_k = sum_d u_d dw_k/dx_d, and with WITH_DADX da_k/dx_e for every e.
// The factors phi_kd are the fp32 ones of the forward's weight product (1 - phi formed in fp32), the products and sums are in A.
template <typename A, int D, bool WITH_DADX>
__device__ __forceinline__ A corner_terms(const float (&phi)[D], const float (&d1)[D], const float (&d2)[D], const A (&u)[D], uint32_t k, A s,
                                          A (&dadx)[D]) {
    A f[D], sd1[D], t[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        const bool up = (k >> d) & 1u;
        f[d] = (A)(up ? phi[d] : 1.0f - phi[d]);
        sd1[d] = up ? (A)d1[d] : -(A)d1[d];
        t[d] = u[d] * sd1[d];
    }
    A a = (A)0;
#pragma unroll
    for (int d = 0; d < D; d++) {
        A p = t[d];
#pragma unroll
        for (int m = 0; m < D; m++)
            if (m != d) p *= f[m];
        a += p;
    }
    if constexpr (WITH_DADX) {
        const A s2 = s * s;
#pragma unroll
        for (int e = 0; e < D; e++) {
            A cross = (A)0;
#pragma unroll
            for (int d = 0; d < D; d++) {
                if (d == e) continue;
                A p = t[d];
#pragma unroll
                for (int m = 0; m < D; m++)
                    if (m != d && m != e) p *= f[m];
                cross += p;
            }
            const bool up = (k >> e) & 1u;
            A diag = u[e] * (up ? (A)d2[e] : -(A)d2[e]);
#pragma unroll
            for (int m = 0; m < D; m++)
                if (m != e) diag *= f[m];
            dadx[e] = s2 * (cross * sd1[e] + diag);
        }
    }
    return a * s;
}

// The coefficient of the record of (a point, corner k) in a level's table gradient, recomputed from the point with the code of the atomic
// paths; x, u: the point's D inputs and, for ORDER 2, its D values of u.  ORDER 1: the weight w_k, corner_weight after locate with the
// call's input map (an fp32 value: exact in double).  ORDER 2: a_k, from the fp32 phi, 1 - phi and phi' of locate_d2 (unit inputs: `im` is
// not read) and u in double -- the sum over d of terms of both signs cancels, and the fp32 form of the atomic path is exact only relative
// to the terms, not to a_k.
template <int D, int ORDER, typename U>
__device__ __forceinline__ double record_coeff(const float* x, const U* u, uint32_t k, float scale, bool align_corners,
                                               uint32_t interp, InputMap im) {
    if constexpr (ORDER == 1) {
        float frac[D], deriv[D];
        uint32_t cell[D];
        locate<D>(x, scale, align_corners, interp, frac, deriv, cell, im);
        return (double)corner_weight<D>(frac, k);
    } else {
        float phi[D], d1[D], d2[D];
        double ud[D], unused[D];
        uint32_t cell[D];
        locate_d2<D>(x, scale, align_corners, interp, phi, d1, d2, cell);
#pragma unroll
        for (int d = 0; d < D; d++) ud[d] = (double)u[d];
        return corner_terms<double, D, false>(phi, d1, d2, ud, k, (double)scale, unused);
    }
}

__device__ __forceinline__ void gg_atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }                 // global_atomic_add_f32
__device__ __forceinline__ void gg_atomic_add_pk(half_t* p, float a, float b) {
    half2_t v = {(half_t)a, (half_t)b};
    (void)__builtin_amdgcn_flat_atomic_fadd_v2f16(reinterpret_cast<half2_t*>(p), v);                          // global_atomic_pk_add_f16
}

// ------------------------------------------------------------------------------------------------
// the u-terms, one pass per (point, level), levels walked in order inside the lane pair
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int C, bool SCATTER>
__global__ __launch_bounds__(GG_THREADS) void k_grid_bwd_bwd(const T* __restrict__ grad, const float* __restrict__ inputs, const T* __restrict__ grid,
                                                             const int32_t* __restrict__ offsets, const T* __restrict__ uin,
                                                             T* __restrict__ grad_grad, T* __restrict__ grad_grid, T* __restrict__ grad_inputs2,
                                                             uint32_t B, uint32_t L, GridLevels lv, uint32_t gridtype, bool align_corners,
                                                             uint32_t interp) {
    using A = typename GGAcc<T>::type;
    constexpr int NJ = 1 << (D - 1);
    // all corners' loads in flight at once where the registers allow it (fully unrolled, D = 5 spills VGPRs and D = 4 SGPRs in the
    // debug-bounds build: one corner / four corners at a time there)
    constexpr int UJ = (NJ * C * (int)sizeof(A) > 128 || D == 5) ? 1 : (D == 4 ? 4 : NJ);
    const uint32_t t = blockIdx.x * GG_THREADS + threadIdx.x;
    const uint32_t b = t >> 1, xb = t & 1u;
    const int pl = (int)(threadIdx.x & 63) >> 1;  // point slot inside the wave
    const bool valid = b < B;                     // (both lanes of a point agree; no early exit: the run merge reads every lane)

    float x[D];
    A u[D], dx[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        x[d] = valid ? inputs[(size_t)b * D + d] : 0.0f;
        u[d] = valid ? (A)uin[(size_t)b * D + d] : (A)0;
        dx[d] = (A)0;
    }

#pragma unroll 1
    for (uint32_t level = 0; level < L; level++) {
        const uint32_t off0 = (uint32_t)offsets[level];
        const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
        const float scale = lv.scale[level];
        LevelIndexer<D> indexer;
        indexer.init(gridtype, align_corners, hashmap_size, lv.res[level]);
        const T* __restrict__ table = grid + (size_t)off0 * C;

        float phi[D], d1[D], d2[D];
        uint32_t cell[D];
#pragma unroll
        for (int d = 0; d < D; d++) { phi[d] = 0.0f; d1[d] = 0.0f; d2[d] = 0.0f; cell[d] = 0u; }
        const bool inside = valid && locate_d2<D>(x, scale, align_corners, interp, phi, d1, d2, cell);
        A g[C], dg[C];
        bool g_nz = false;
#pragma unroll
        for (int c = 0; c < C; c++) { g[c] = (A)0; dg[c] = (A)0; }
        if (inside) load_row<T, A, C>(grad + ((size_t)level * B + b) * C, g);
#pragma unroll
        for (int c = 0; c < C; c++) g_nz = g_nz || (g[c] != (A)0);

#pragma unroll UJ
        for (int j = 0; j < NJ; j++) {
            const uint32_t k = xb | ((uint32_t)j << 1);
            uint32_t pg[D];
#pragma unroll
            for (int d = 0; d < D; d++) pg[d] = cell[d] + ((k >> d) & 1u);
            const uint32_t idx = inside ? indexer(pg) : 0u;
            NGP_BOUNDS(idx < hashmap_size);
            A e[C];
#pragma unroll
            for (int c = 0; c < C; c++) e[c] = (A)0;
            if (inside) load_row<T, A, C>(table + (size_t)idx * C, e);
            A dadx[D];
            const A a = corner_terms<A, D, true>(phi, d1, d2, u, k, (A)scale, dadx);
            A G = (A)0;
#pragma unroll
            for (int c = 0; c < C; c++) {
                G = gg_fma(g[c], e[c], G);
                dg[c] = gg_fma(a, e[c], dg[c]);
            }
#pragma unroll
            for (int d = 0; d < D; d++) dx[d] = gg_fma(dadx[d], G, dx[d]);

            if constexpr (SCATTER) {
                float v[C];
#pragma unroll
                for (int c = 0; c < C; c++) v[c] = a * g[c];
                const bool live = inside && g_nz && a != (A)0;
                // runs of equal destinations over the wave's point slots (slot pl and pl - 1 share the lane class xb: lanes 2 apart)
                const uint32_t prev_idx = __shfl_up(idx, 2, 64);
                const int prev_live = __shfl_up((int)live, 2, 64);
                const bool same = live && pl > 0 && prev_live != 0 && prev_idx == idx;
                bool issue = live;
                if (__any(same)) {
                    bool reached = !same;  // the scan of this lane has reached the head of its run
#pragma unroll
                    for (int o = 1; o < 32; o <<= 1) {
                        const int r_o = __shfl_up((int)reached, 2 * o, 64);
                        const bool take = !reached && pl >= o;
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            const float tv = __shfl_up(v[c], 2 * o, 64);
                            if (take) v[c] += tv;
                        }
                        if (take) reached = r_o != 0;
                    }
                    const int next_same = __shfl_down((int)same, 2, 64);
                    issue = live && (pl == 31 || !next_same);  // the last lane of a run holds the run total
                }
                if (issue) {
                    T* dst = grad_grid + ((size_t)off0 + idx) * C;
                    if constexpr (sizeof(T) == 2) {
#pragma unroll
                        for (int c = 0; c < C; c += 2) gg_atomic_add_pk(reinterpret_cast<half_t*>(dst) + c, v[c], v[c + 1]);
                    } else {
#pragma unroll
                        for (int c = 0; c < C; c++) gg_atomic_add(reinterpret_cast<float*>(dst) + c, v[c]);
                    }
                }
            }
        }
        // the two half sums of the point (both lanes form the same bits)
#pragma unroll
        for (int c = 0; c < C; c++) dg[c] += __shfl_xor(dg[c], 1, 64);
        if (grad_grad && valid && xb == 0u) {
            T* out = grad_grad + ((size_t)level * B + b) * C;
#pragma unroll
            for (int c = 0; c < C; c++) out[c] = (T)dg[c];
        }
    }
#pragma unroll
    for (int d = 0; d < D; d++) dx[d] += __shfl_xor(dx[d], 1, 64);
    if (grad_inputs2 && valid && xb == 0u) {
#pragma unroll
        for (int d = 0; d < D; d++) grad_inputs2[(size_t)b * D + d] = (T)dx[d];
    }
}

}  // namespace ngp
