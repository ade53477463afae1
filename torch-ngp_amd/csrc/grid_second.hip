// Second-order backward of the grid encoder for gfx950 (MI355X): the backward of the first backward, so that a loss on d enc / d x
// (eikonal / SDF regularisers: torch.autograd.grad(sdf, x, create_graph=True)) trains the table, the upstream gradient and the inputs.
//
// Per level l and point b (positions, cells, phi, phi', phi'' from the fp32 inputs exactly as locate() forms them, grid_index.h:
// locate_d2), the first backward computed gE[i_k] += w_k g and gx[b] = sum_{l,c} g J; its backward receives u = dL2/dgx [B,D].  With
//   a_k = sum_d u_d dw_k/dx_d                                   (the derivative of corner k's weight along u)
//   da_k/dx_e = s^2 sgn_ke phi'_e sum_{d != e} u_d sgn_kd phi'_d prod_{m != d,e} phi_km  +  s^2 u_e sgn_ke phi''_e prod_{m != e} phi_km
// the three u-terms come out of ONE walk over the point's corners (DESIGN.md "Second order through the grid encoder"):
//   dL2/dE[i_k, c] += a_k g[l,b,c]                                (scatter)
//   dL2/dg[l,b,c]   = sum_k a_k E[i_k, c]                         (gather, per point)
//   dL2/dx[b,e]    += sum_k da_k/dx_e sum_c g[l,b,c] E[i_k, c]    (gather, per point, summed over the levels inside the lane)
// The v-terms (v = dL2/dgE) are the forward and the first-order input backward on the table v: the existing entries (gridencoder/grid.py).
//
// Layout: two lanes per point, lane parity xb owns the 2^(D-1) corners whose first coordinate is the cell's lower / upper vertex -- the two
// entries of a corner pair are neighbours in memory (dense levels by construction, hashed levels because the first prime is 1), so a
// scatter instruction touches one line per point instead of two.  The two half sums of the per-point results are combined with one
// lane swap (a + b == b + a: both lanes hold the same bits) and the levels are walked in order: dL2/dg and dL2/dx are deterministic, no
// atomics, in every dtype.  The scatter:
//   * fp32 tables: global_atomic_add_f32 (unsafeAtomicAdd); fp16 tables (even C): global_atomic_pk_add_f16; before the atomic, runs of
//     equal destinations over the point slots of a wave are summed (segmented scan, issued only when a wave has such a run);
//   * fp64 tables: bit-reproducible.  The records and the stable radix sort of the first-order fp64 backward (fp64.hip,
//     f64_grid_sort_level), then one lane per run of equal entries sums a_k g in slot order in fp64 and adds the sum once.
#include "common.h"
#include "grid_index.h"
#include "fp64.h"
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

// ------------------------------------------------------------------------------------------------
// fp64 tables: the dL2/dE scatter, bit-reproducible.  One lane per run of equal entries of the sorted records of one level (fp64.hip:
// f64_grid_sort_level; the run's first record), the contributions a_k g in slot order, summed in fp64, added once.
// ------------------------------------------------------------------------------------------------
template <int D, int C>
__global__ __launch_bounds__(GG_THREADS) void k_f64_grid_bwd_bwd_sum(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n,
                                                                     const double* __restrict__ grad, const float* __restrict__ inputs,
                                                                     const double* __restrict__ uin, const int32_t* __restrict__ offsets,
                                                                     double* __restrict__ grad_grid, uint32_t B, uint32_t level, float scale,
                                                                     bool align_corners, uint32_t interp) {
    constexpr uint32_t NO_ENTRY = 0xffffffffu;  // (fp64.hip: a record of a point outside [0,1]^D)
    for (uint32_t i = blockIdx.x * GG_THREADS + threadIdx.x; i < n; i += gridDim.x * GG_THREADS) {
        const uint32_t e = keys[i];
        if (e == NO_ENTRY || (i > 0u && keys[i - 1u] == e)) continue;
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 0.0;
        for (uint32_t j = i; j < n && keys[j] == e; j++) {
            const uint32_t slot = vals[j], b = slot >> D, k = slot & ((1u << D) - 1u);
            NGP_BOUNDS(b < B);
            float phi[D], d1[D], d2[D];
            uint32_t cell[D];
            locate_d2<D>(inputs + (size_t)b * D, scale, align_corners, interp, phi, d1, d2, cell);
            double u[D], unused[D];
#pragma unroll
            for (int d = 0; d < D; d++) u[d] = uin[(size_t)b * D + d];
            const double a = corner_terms<double, D, false>(phi, d1, d2, u, k, (double)scale, unused);
            const double* g = grad + ((size_t)level * B + b) * C;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = __builtin_fma(a, g[c], acc[c]);
        }
        const uint32_t off0 = (uint32_t)offsets[level];
        NGP_BOUNDS(e < (uint32_t)offsets[level + 1] - off0);
        double* dst = grad_grid + ((size_t)off0 + e) * C;
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] += acc[c];
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
struct GGArgs {
    const void* grad;
    const float* inputs;
    const void* embeddings;
    const int32_t* offsets;
    const void* u;
    void* grad_grad;
    void* grad_embeddings;
    void* grad_inputs2;
    uint32_t B, L, gridtype, interp;
    bool align_corners;
    GridLevels lv;
    void* workspace;
};

template <typename T, int D, int C>
static int launch_bwd_bwd(const GGArgs& a, hipStream_t st) {
    constexpr bool SCATTER = sizeof(T) != 8;
    if constexpr (sizeof(T) == 2 && (C & 1)) {
        return NGP_ERR_INVALID;  // (refused by the entry point)
    } else {
        if (SCATTER || a.grad_grad || a.grad_inputs2) {
            const uint32_t blocks = (uint32_t)cdiv64(2ull * a.B, GG_THREADS);
            hipLaunchKernelGGL((k_grid_bwd_bwd<T, D, C, SCATTER>), dim3(blocks), dim3(GG_THREADS), 0, st, (const T*)a.grad, a.inputs,
                               (const T*)a.embeddings, a.offsets, (const T*)a.u, (T*)a.grad_grad, (T*)a.grad_embeddings, (T*)a.grad_inputs2, a.B, a.L,
                               a.lv, a.gridtype, a.align_corners, a.interp);
            const int rc = check_launch("grid_encode_backward_backward");
            if (rc) return rc;
        }
        if constexpr (!SCATTER) {
            const uint32_t n = a.B << D;
            for (uint32_t level = 0; level < a.L; level++) {
                const uint32_t *keys, *vals;
                f64_grid_sort_level((uint32_t)D, a.inputs, a.offsets, a.B, level, a.lv.scale[level], a.lv.res[level], a.gridtype, a.align_corners,
                                    a.interp, a.workspace, &keys, &vals, st);
                hipLaunchKernelGGL((k_f64_grid_bwd_bwd_sum<D, C>), dim3(grid_blocks(n, GG_THREADS)), dim3(GG_THREADS), 0, st, keys, vals, n, (const double*)a.grad,
                                   a.inputs, (const double*)a.u, a.offsets, (double*)a.grad_embeddings, a.B, level, a.lv.scale[level], a.align_corners,
                                   a.interp);
                const int rc = check_launch("grid_encode_backward_backward(fp64)");
                if (rc) return rc;
            }
        }
        return NGP_OK;
    }
}

template <typename T>
static int dispatch_bwd_bwd(uint32_t D, uint32_t C, const GGArgs& a, hipStream_t st) {
    NGP_DISPATCH_DC(D, C, launch_bwd_bwd<T, D_, C_>(a, st))
    set_error("grid_encode_backward_backward: unsupported (D=%u, C=%u)", D, C);
    return NGP_ERR_INVALID;
}

}  // namespace ngp

using namespace ngp;

extern "C" size_t ngp_grid_backward_backward_workspace_bytes(const int32_t* offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L, int dtype) {
    (void)offsets_host;
    (void)C;
    // fp16 / fp32 tables scatter with atomics and need no scratch; fp64 sorts one level's records at a time (B and D alone)
    if (dtype != NGP_F64 || L < 1 || L > NGP_MAX_LEVELS) return 0;
    return f64_grid_backward_workspace_bytes(B, D);
}

extern "C" int ngp_grid_encode_backward_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                                 const void* grad_grad_inputs, void* grad_grad, void* grad_embeddings, void* grad_inputs2, uint32_t B,
                                                 uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                                 uint32_t interp, int dtype, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    const char* fn = "grid_encode_backward_backward";
    NGP_REQUIRE(D >= 2 && D <= 5, NGP_ERR_INVALID, "%s: GridEncoding: input dim D must be 2, 3, 4 or 5 (got %u)", fn, D);
    NGP_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8, NGP_ERR_INVALID, "%s: GridEncoding: C must be 1, 2, 4, or 8. (got %u)", fn, C);
    NGP_REQUIRE(L >= 1 && L <= NGP_MAX_LEVELS, NGP_ERR_INVALID, "%s: number of levels must be in [1, %d] (got %u)", fn, NGP_MAX_LEVELS, L);
    NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F16 || dtype == NGP_F64, NGP_ERR_INVALID, "%s: embeddings must be float32, float16 or float64",
                fn);
    NGP_REQUIRE(!(dtype == NGP_F16 && (C & 1u)), NGP_ERR_INVALID,
                "%s: float16 tables need an even C (packed fp16 atomics; autocast only makes fp16 tables for even C), got C=%u", fn, C);
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && inputs && embeddings && offsets && grad_grad_inputs && grad_embeddings, NGP_ERR_INVALID, "%s: NULL tensor", fn);
    NGP_REQUIRE(B < (1u << 31), NGP_ERR_INVALID, "%s: B must be below 2^31 (got %u)", fn, B);
    if (dtype == NGP_F64) {
        NGP_REQUIRE(((uint64_t)B << D) <= (1ull << 31), NGP_ERR_INVALID, "%s: fp64: B * 2^D must not exceed 2^31 (B=%u, D=%u)", fn, B, D);
        const size_t need = f64_grid_backward_workspace_bytes(B, D);
        NGP_REQUIRE(workspace && workspace_bytes >= need, NGP_ERR_INVALID,
                    "%s: fp64 needs a workspace of %zu bytes (ngp_grid_backward_backward_workspace_bytes), got %zu", fn, need,
                    workspace ? workspace_bytes : (size_t)0);
        NGP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, NGP_ERR_INVALID, "%s: fp64: workspace must be 256-byte aligned", fn);
    }
    GGArgs a;
    a.grad = grad;
    a.inputs = inputs;
    a.embeddings = embeddings;
    a.offsets = offsets;
    a.u = grad_grad_inputs;
    a.grad_grad = grad_grad;
    a.grad_embeddings = grad_embeddings;
    a.grad_inputs2 = grad_inputs2;
    a.B = B;
    a.L = L;
    a.gridtype = gridtype;
    a.interp = interp;
    a.align_corners = align_corners != 0;
    a.workspace = workspace;
    fill_levels(a.lv, L, S, H);
    const hipStream_t st = as_stream(stream);
    if (dtype == NGP_F16) return dispatch_bwd_bwd<half_t>(D, C, a, st);
    if (dtype == NGP_F32) return dispatch_bwd_bwd<float>(D, C, a, st);
    return dispatch_bwd_bwd<double>(D, C, a, st);
}
