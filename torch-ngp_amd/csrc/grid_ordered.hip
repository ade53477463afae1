// Ordered scatter of the grid encoder's table gradient for gfx950 (MI355X): fp32 and fp16 tables, first order (w_k g) and second order
// (a_k g), bit-reproducible, no float atomics.  Opt-in: ngp_grid_encode_backward_ordered and
// ngp_grid_encode_backward_backward_ordered; the entries of gridencoder.hip / grid_second.hip run what they always ran.
//
// Per level:
//   records   one per (point, corner), sorted by table entry, equal entries in slot order: the record sort of grid_records.h, which the
//             fp64 backwards (fp64.hip) use as well;
//   sum       THE ORDER (part of the contract, a function of the sorted array alone).  The array is cut into tiles of 64 records, one wave
//             each.  A fragment is a tile's run of records of one entry; the lane at its head adds the fragment's contributions left to
//             right in fp32, starting from the first (at most 63 additions).  A fragment whose run lies inside the tile is added to the
//             entry: dst = T(float(dst) + sum).  A fragment whose run goes on beyond the tile's first or last record becomes a record
//             (entry, partial sum) of the next array, which has two slots per tile: slot 2t for the fragment that crosses tile t's left
//             edge, slot 2t + 1 for the one that crosses its right edge.  A fragment that crosses both fills slot 2t, and slot 2t + 1
//             repeats the entry with the ABSENT mark (it keeps the run contiguous and is skipped by the sum); a slot without a fragment is
//             NONE.  The same step runs on that array, and on the next, until an array fits one tile: ceil-log-many launches whose number
//             and sizes follow from n alone, so the call reads nothing back and can be captured in a graph.
// The contribution of a record: its coefficient recomputed from the slot (grid_second.h: record_coeff, w_k or a_k in double), rounded to
// fp32 once, one fp32 product with the gradient value.
#include "common.h"
#include "grid_index.h"
#include "grid_records.h"
#include "grid_second.h"
#include <math.h>

namespace ngp {

constexpr int ORD_THREADS = 256;
constexpr uint32_t ORD_TILE = 64;              // records per tile of the sum = lanes of a wave
constexpr uint32_t ORD_NONE = 0xffffffffu;     // no record (an empty slot, a record of a point outside the level)
constexpr uint32_t ORD_ABSENT = 0x80000000u;   // the record repeats its left neighbour's entry and carries no value
constexpr int ORD_MAX_ARRAYS = 8;              // arrays of partial sums: 5 for the largest call (2^31 records)

// ------------------------------------------------------------------------------------------------
// the sum of one tile (one wave): THE ORDER of the header
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }
__device__ __forceinline__ float lane_f32(float v, uint32_t lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)lane));
}
// a record's entry without the ABSENT mark (NONE stays NONE)
__device__ __forceinline__ uint32_t entry_of(uint32_t key) { return key == ORD_NONE ? ORD_NONE : key & ~ORD_ABSENT; }

__device__ __forceinline__ float add_to(float dst, float sum) { return dst + sum; }
__device__ __forceinline__ half_t add_to(half_t dst, float sum) { return to_half_rne((float)dst + sum); }

// key / v: this lane's record of tile `tile` (v is read only where key carries a value); prev_last / next_first: the entries of the records
// beside the tile (NONE at the ends of the array); out_keys == nullptr: the array is one tile, nothing crosses an edge
template <typename T, int C>
__device__ __forceinline__ void ord_tile_sum(uint32_t key, const float (&v)[C], uint32_t prev_last, uint32_t next_first, uint32_t tile,
                                             uint32_t* __restrict__ out_keys, float* __restrict__ out_vals, T* __restrict__ table,
                                             uint32_t level_size) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = entry_of(key);
    const uint32_t e_prev = __shfl_up(e, 1, 64);
    // (an ABSENT record follows the record it repeats inside the same tile: never a head)
    const bool head = e != ORD_NONE && (lane == 0u || e_prev != e);
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = v[c];
    if (__any(e != ORD_NONE && !head)) {
        // (not unrolled: the unrolled loop reads every lane ahead into scalar registers and spills them)
#pragma unroll 1
        for (uint32_t j = 1; j < ORD_TILE; j++) {
            // (key_j == e: record j carries a value of this lane's entry; the records of an entry are neighbours)
            const bool add = head && j > lane && lane_u32(key, j) == e;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float vj = lane_f32(v[c], j);
                acc[c] = add ? acc[c] + vj : acc[c];
            }
        }
    }
    const bool cross_left = head && lane == 0u && prev_last == e;
    const bool cross_right = head && lane_u32(e, ORD_TILE - 1u) == e && next_first == e;
    if (head && !cross_left && !cross_right) {
        NGP_BOUNDS(e < level_size);
        T* dst = table + (size_t)e * C;
#pragma unroll
        for (int c = 0; c < C; c++) dst[c] = add_to(dst[c], acc[c]);
    }
    if (out_keys == nullptr) return;
    const bool any_right = __any(cross_right);
    if (lane == 0u) {
        out_keys[2u * tile] = cross_left ? e : ORD_NONE;
        if (!any_right) out_keys[2u * tile + 1u] = ORD_NONE;
    }
    if (cross_left || cross_right) {
        // (both: the fragment is the whole tile, lane 0 holds it)
        const uint32_t slot = 2u * tile + (cross_left ? 0u : 1u);
#pragma unroll
        for (int c = 0; c < C; c++) out_vals[(size_t)slot * C + c] = acc[c];
        if (cross_right) out_keys[2u * tile + 1u] = cross_left ? (e | ORD_ABSENT) : e;
    }
}

// the first array: the sorted records, contributions recomputed from the slots.  ORDER 1: w_k g, ORDER 2: a_k g
template <typename T, int D, int C, int ORDER>
__global__ __launch_bounds__(ORD_THREADS) void k_ord_sum_records(const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ vals0,
                                                                 const uint32_t* __restrict__ keys1, const uint32_t* __restrict__ vals1, uint32_t n,
                                                                 const T* __restrict__ grad, const float* __restrict__ inputs,
                                                                 const T* __restrict__ uin, const int32_t* __restrict__ offsets,
                                                                 T* __restrict__ grad_grid, uint32_t B, uint32_t level, float scale,
                                                                 bool align_corners, uint32_t interp, InputMap im, uint32_t* __restrict__ out_keys,
                                                                 float* __restrict__ out_vals) {
    const uint32_t level_size = level_size_of(offsets, level);
    const bool odd = rec_sorted_side(level_size) != 0u;
    const uint32_t* __restrict__ keys = odd ? keys1 : keys0;
    const uint32_t* __restrict__ vals = odd ? vals1 : vals0;
    const uint32_t tile = (blockIdx.x * ORD_THREADS + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (tile >= (n + ORD_TILE - 1u) / ORD_TILE) return;   // (whole waves)
    const uint32_t r = tile * ORD_TILE + lane;
    uint32_t key = r < n ? keys[r] : ORD_NONE;
    if (key >= level_size) key = ORD_NONE;
    uint32_t prev_last = ORD_NONE, next_first = ORD_NONE;
    if (tile > 0u) prev_last = keys[tile * ORD_TILE - 1u];
    if (n - tile * ORD_TILE > ORD_TILE) next_first = keys[(tile + 1u) * ORD_TILE];
    if (prev_last >= level_size) prev_last = ORD_NONE;
    if (next_first >= level_size) next_first = ORD_NONE;

    float v[C];
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = 0.0f;
    if (key != ORD_NONE) {
        const uint32_t slot = vals[r], b = slot >> D, k = slot & ((1u << D) - 1u);
        NGP_BOUNDS(b < B);
        float g[C];
        load_row<T, float, C>(grad + ((size_t)level * B + b) * C, g);
        // (rounded once; w_k is an fp32 value already.  The bound of the tests is relative to |a_k g|)
        const float w = (float)record_coeff<D, ORDER>(inputs + (size_t)b * D, ORDER == 2 ? uin + (size_t)b * D : nullptr, k, scale, align_corners,
                                                      interp, im);
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = w * g[c];
    }
    ord_tile_sum<T, C>(key, v, prev_last, next_first, tile, out_keys, out_vals, grad_grid + (size_t)(uint32_t)offsets[level] * C, level_size);
}

// the later arrays: (entry, partial sum) records
template <typename T, int C>
__global__ __launch_bounds__(ORD_THREADS) void k_ord_sum_partials(const uint32_t* __restrict__ in_keys, const float* __restrict__ in_vals, uint32_t m,
                                                                  const int32_t* __restrict__ offsets, T* __restrict__ grad_grid, uint32_t level,
                                                                  uint32_t* __restrict__ out_keys, float* __restrict__ out_vals) {
    const uint32_t tile = (blockIdx.x * ORD_THREADS + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (tile >= (m + ORD_TILE - 1u) / ORD_TILE) return;   // (whole waves)
    const uint32_t r = tile * ORD_TILE + lane;
    const uint32_t key = r < m ? in_keys[r] : ORD_NONE;
    uint32_t prev_last = ORD_NONE, next_first = ORD_NONE;
    if (tile > 0u) prev_last = entry_of(in_keys[tile * ORD_TILE - 1u]);
    if (m - tile * ORD_TILE > ORD_TILE) next_first = entry_of(in_keys[(tile + 1u) * ORD_TILE]);
    float v[C];
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = 0.0f;
    if (key != ORD_NONE && !(key & ORD_ABSENT)) load_row<float, float, C>(in_vals + (size_t)r * C, v);
    ord_tile_sum<T, C>(key, v, prev_last, next_first, tile, out_keys, out_vals, grad_grid + (size_t)(uint32_t)offsets[level] * C,
                       level_size_of(offsets, level));
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the workspace of a call: a function of (B, D, C) alone.  The record sort's part (grid_records.h: rec_layout), then the arrays of partial
// sums: m_1 = 2 ceil(n / 64) records, m_2 = 2 ceil(m_1 / 64), ... until one fits a tile
struct OrdLayout {
    size_t total;
    uint32_t n_arrays;                  // arrays of partial sums (the sum launches are n_arrays + 1)
    uint32_t m[ORD_MAX_ARRAYS];
    size_t part_keys[ORD_MAX_ARRAYS], part_vals[ORD_MAX_ARRAYS];
};

static OrdLayout ord_layout(uint32_t B, uint32_t D, uint32_t C) {
    OrdLayout w = {};
    const RecLayout sort = rec_layout(B, D);
    size_t at = sort.bytes;
    for (uint32_t m = sort.n; m > ORD_TILE; w.n_arrays++) {
        m = 2u * cdiv(m, ORD_TILE);
        w.m[w.n_arrays] = m;
        w.part_keys[w.n_arrays] = at;
        at += align256((uint64_t)m * sizeof(uint32_t));
        w.part_vals[w.n_arrays] = at;
        at += align256((uint64_t)m * C * sizeof(float));
    }
    w.total = at;
    return w;
}

struct OrdArgs {
    const void* grad;
    const float* inputs;
    const int32_t* offsets;
    const void* u;           // second order only
    void* grad_embeddings;
    uint32_t B, L, gridtype, interp;
    bool align_corners;
    InputMap im;
    GridLevels lv;
    void* workspace;
};

template <typename T, int D, int C, int ORDER>
static int launch_ordered_scatter(const OrdArgs& a, const char* what, hipStream_t st) {
    const OrdLayout w = ord_layout(a.B, D, C);
    char* ws = (char*)a.workspace;
    auto part_keys = [&](uint32_t i) { return i < w.n_arrays ? (uint32_t*)(ws + w.part_keys[i]) : nullptr; };
    auto part_vals = [&](uint32_t i) { return i < w.n_arrays ? (float*)(ws + w.part_vals[i]) : nullptr; };
    for (uint32_t level = 0; level < a.L; level++) {
        const RecSides r = rec_sort_level(D, a.inputs, a.offsets, a.B, level, a.lv.scale[level], a.lv.res[level], a.gridtype, a.align_corners,
                                          a.interp, a.im, a.workspace, st);
        // one wave per tile of 64 records, the exact grid (the order does not depend on it: a tile is a fixed slice of the array)
        NGP_LAUNCH((k_ord_sum_records<T, D, C, ORDER>), dim3((uint32_t)cdiv64((uint64_t)cdiv(r.n, ORD_TILE) * ORD_TILE, ORD_THREADS)),
                           dim3(ORD_THREADS), 0, st, r.keys[0], r.vals[0], r.keys[1], r.vals[1], r.n, (const T*)a.grad, a.inputs, (const T*)a.u,
                           a.offsets, (T*)a.grad_embeddings, a.B, level, a.lv.scale[level], a.align_corners, a.interp, a.im, part_keys(0), part_vals(0));
        for (uint32_t i = 0; i < w.n_arrays; i++)
            NGP_LAUNCH((k_ord_sum_partials<T, C>), dim3((uint32_t)cdiv64((uint64_t)cdiv(w.m[i], ORD_TILE) * ORD_TILE, ORD_THREADS)),
                               dim3(ORD_THREADS), 0, st, part_keys(i), part_vals(i), w.m[i], a.offsets, (T*)a.grad_embeddings, level, part_keys(i + 1),
                               part_vals(i + 1));
        const int rc = check_launch(what);
        if (rc) return rc;
    }
    return NGP_OK;
}

// what both entries check before any launch; B == 0 is left to the callers (a no-op once these pass)
static int check_ordered_args(const char* fn, uint32_t B, uint32_t D, uint32_t C, uint32_t L, int dtype, const char* f64_entry) {
    NGP_REQUIRE(D >= 2 && D <= 5, NGP_ERR_INVALID, "%s: GridEncoding: input dim D must be 2, 3, 4 or 5 (got %u)", fn, D);
    NGP_REQUIRE(C == 1 || C == 2 || C == 4 || C == 8, NGP_ERR_INVALID, "%s: GridEncoding: C must be 1, 2, 4, or 8. (got %u)", fn, C);
    NGP_REQUIRE(L >= 1 && L <= NGP_MAX_LEVELS, NGP_ERR_INVALID, "%s: number of levels must be in [1, %d] (got %u)", fn, NGP_MAX_LEVELS, L);
    NGP_REQUIRE(dtype != NGP_F64, NGP_ERR_INVALID, "%s: float64 is not provided by this entry point (%s is bit-reproducible for float64)", fn,
                f64_entry);
    NGP_REQUIRE(dtype == NGP_F32 || dtype == NGP_F16, NGP_ERR_INVALID, "%s: embeddings must be float32 or float16", fn);
    (void)B;
    return NGP_OK;
}

// the launch arguments of both entries (u: second order only; bound: the first order's fused input mapping, <= 0 for unit coordinates)
static OrdArgs ordered_args(const void* grad, const float* inputs, const int32_t* offsets, const void* u, void* grad_embeddings, uint32_t B,
                            uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, float bound, void* workspace) {
    OrdArgs a = {};
    a.grad = grad;
    a.inputs = inputs;
    a.offsets = offsets;
    a.u = u;
    a.grad_embeddings = grad_embeddings;
    a.B = B;
    a.L = L;
    a.gridtype = gridtype;
    a.interp = interp;
    a.align_corners = align_corners != 0;
    a.im = make_input_map(bound);
    a.workspace = workspace;
    fill_levels(a.lv, L, S, H);
    return a;
}

static int check_ordered_workspace(const char* fn, uint32_t B, uint32_t D, uint32_t C, int dtype, const void* workspace, size_t workspace_bytes) {
    return rec_check_workspace(fn, "", "ngp_grid_ordered_workspace_bytes", B, D, ngp_grid_ordered_workspace_bytes(B, D, C, dtype), workspace,
                               workspace_bytes);
}

template <typename T>
static int dispatch_ordered_first(uint32_t D, uint32_t C, const OrdArgs& a, hipStream_t st) {
    NGP_DISPATCH_DC(D, C, launch_ordered_scatter<T, D_, C_, 1>(a, "grid_encode_backward_ordered", st))
    return NGP_ERR_INVALID;   // (D and C are checked by the entry)
}

template <typename T, int D, int C>
static int launch_ordered_second(const OrdArgs& a, const void* embeddings, void* grad_grad, void* grad_inputs2, hipStream_t st) {
    const char* what = "grid_encode_backward_backward_ordered";
    if (grad_grad || grad_inputs2) {
        // the gather-only form of the atomic entry's kernel: grad_grad and grad_inputs2 with its bits
        const uint32_t blocks = (uint32_t)cdiv64(2ull * a.B, GG_THREADS);
        NGP_LAUNCH((k_grid_bwd_bwd<T, D, C, false>), dim3(blocks), dim3(GG_THREADS), 0, st, (const T*)a.grad, a.inputs, (const T*)embeddings,
                           a.offsets, (const T*)a.u, (T*)grad_grad, (T*)nullptr, (T*)grad_inputs2, a.B, a.L, a.lv, a.gridtype, a.align_corners,
                           a.interp);
        const int rc = check_launch(what);
        if (rc) return rc;
    }
    return launch_ordered_scatter<T, D, C, 2>(a, what, st);
}

template <typename T>
static int dispatch_ordered_second(uint32_t D, uint32_t C, const OrdArgs& a, const void* embeddings, void* grad_grad, void* grad_inputs2,
                                   hipStream_t st) {
    NGP_DISPATCH_DC(D, C, launch_ordered_second<T, D_, C_>(a, embeddings, grad_grad, grad_inputs2, st))
    return NGP_ERR_INVALID;   // (D and C are checked by the entry)
}

}  // namespace ngp

using namespace ngp;

extern "C" size_t ngp_grid_ordered_workspace_bytes(uint32_t B, uint32_t D, uint32_t C, int dtype) {
    // (fp16 and fp32 tables: the same scratch, the partial sums are fp32 for both)
    if (B == 0 || D < 2 || D > 5 || !(C == 1 || C == 2 || C == 4 || C == 8) || !(dtype == NGP_F32 || dtype == NGP_F16)) return 0;
    if (((uint64_t)B << D) > (1ull << 31)) return 0;
    return ord_layout(B, D, C).total;
}

extern "C" int ngp_grid_encode_backward_ordered(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                                void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                                const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                                float bound, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    (void)embeddings;
    const char* fn = "grid_encode_backward_ordered";
    int rc = check_ordered_args(fn, B, D, C, L, dtype, "ngp_grid_encode_backward_ws");
    if (rc) return rc;
    NGP_REQUIRE(!(bound > 0.0f && dy_dx), NGP_ERR_INVALID, "%s: the fused input mapping does not provide grad_inputs", fn);
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && inputs && offsets && grad_embeddings, NGP_ERR_INVALID, "%s: NULL tensor", fn);
    NGP_REQUIRE(!dy_dx == !grad_inputs, NGP_ERR_INVALID, "%s: dy_dx and grad_inputs must both be given or both be NULL", fn);
    rc = check_ordered_workspace(fn, B, D, C, dtype, workspace, workspace_bytes);
    if (rc) return rc;
    const OrdArgs a = ordered_args(grad, inputs, offsets, nullptr, grad_embeddings, B, L, S, H, gridtype, align_corners, interp, bound, workspace);
    const hipStream_t st = as_stream(stream);
    rc = dtype == NGP_F16 ? dispatch_ordered_first<half_t>(D, C, a, st) : dispatch_ordered_first<float>(D, C, a, st);
    if (rc || !dy_dx) return rc;
    // the input term: the kernel of ngp_grid_encode_backward (grid_index.h), the same bits
    if (dtype == NGP_F16)
        NGP_LAUNCH((k_grid_input_backward<half_t>), dim3(cdiv(B * D, 256)), dim3(256), 0, st, (const half_t*)grad, (const half_t*)dy_dx,
                           (half_t*)grad_inputs, B, L, D, C);
    else
        NGP_LAUNCH((k_grid_input_backward<float>), dim3(cdiv(B * D, 256)), dim3(256), 0, st, (const float*)grad, (const float*)dy_dx,
                           (float*)grad_inputs, B, L, D, C);
    return check_launch("grid_encode_backward_ordered(input)");
}

extern "C" int ngp_grid_encode_backward_backward_ordered(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                                         const void* grad_grad_inputs, void* grad_grad, void* grad_embeddings, void* grad_inputs2,
                                                         uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                                         int align_corners, uint32_t interp, int dtype, void* workspace, size_t workspace_bytes,
                                                         ngp_stream_t stream) {
    const char* fn = "grid_encode_backward_backward_ordered";
    int rc = check_ordered_args(fn, B, D, C, L, dtype, "ngp_grid_encode_backward_backward");
    if (rc) return rc;
    if (B == 0) return NGP_OK;
    NGP_REQUIRE(grad && inputs && embeddings && offsets && grad_grad_inputs && grad_embeddings, NGP_ERR_INVALID, "%s: NULL tensor", fn);
    rc = check_ordered_workspace(fn, B, D, C, dtype, workspace, workspace_bytes);
    if (rc) return rc;
    const OrdArgs a = ordered_args(grad, inputs, offsets, grad_grad_inputs, grad_embeddings, B, L, S, H, gridtype, align_corners, interp, 0.0f,
                                   workspace);
    const hipStream_t st = as_stream(stream);
    return dtype == NGP_F16 ? dispatch_ordered_second<half_t>(D, C, a, embeddings, grad_grad, grad_inputs2, st)
                            : dispatch_ordered_second<float>(D, C, a, embeddings, grad_grad, grad_inputs2, st);
}
