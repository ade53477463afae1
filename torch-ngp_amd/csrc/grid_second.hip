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
//   * fp64 tables: bit-reproducible, left to fp64.hip (f64_grid_table_grad, order 2): the record sort and run sum of the first-order fp64
//     backward with the coefficient a_k.
#include "common.h"
#include "grid_index.h"
#include "grid_second.h"
#include "fp64.h"
#include <math.h>

namespace ngp {

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
            NGP_LAUNCH((k_grid_bwd_bwd<T, D, C, SCATTER>), dim3(blocks), dim3(GG_THREADS), 0, st, (const T*)a.grad, a.inputs,
                               (const T*)a.embeddings, a.offsets, (const T*)a.u, (T*)a.grad_grad, (T*)a.grad_embeddings, (T*)a.grad_inputs2, a.B, a.L,
                               a.lv, a.gridtype, a.align_corners, a.interp);
            const int rc = check_launch("grid_encode_backward_backward");
            if (rc) return rc;
        }
        if constexpr (!SCATTER)
            return f64_grid_table_grad(2, a.grad, a.inputs, a.offsets, a.u, a.grad_embeddings, a.B, D, C, a.L, a.lv, a.gridtype, a.align_corners,
                                       a.interp, a.workspace, st);
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
        const int rc = f64_grid_check_workspace(fn, "ngp_grid_backward_backward_workspace_bytes", B, D, workspace, workspace_bytes);
        if (rc) return rc;
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
