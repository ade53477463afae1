// Ordered scatter of the grid encoder's table gradient for gfx950 (MI355X): fp32 and fp16 tables, first order (w_k g) and second order
// (a_k g), bit-reproducible, no float atomics.  Opt-in: ngp_grid_encode_backward_ordered and
// ngp_grid_encode_backward_backward_ordered; the entries of gridencoder.hip / grid_second.hip run what they always ran.
//
// Per level:
//   records   one per (point, corner), n = B << D: key = the entry inside the level (level_size for a point outside [0,1]^D: sorts last,
//             contributes nothing), value = the slot b << D | k;
//   sort      stable LSD radix sort on the key, 8 bits a pass.  Four passes are launched (the host does not know the level sizes: the
//             offsets are device memory, and nothing is read back), a pass above bit_length(level_size) returns at once: 2 or 3 passes do
//             work for the tables in use.  The sorted records are in buffer (passes that worked) & 1;
//   sum       THE ORDER (part of the contract, a function of the sorted array alone).  The array is cut into tiles of 64 records, one wave
//             each.  A fragment is a tile's run of records of one entry; the lane at its head adds the fragment's contributions left to
//             right in fp32, starting from the first (at most 63 additions).  A fragment whose run lies inside the tile is added to the
//             entry: dst = T(float(dst) + sum).  A fragment whose run goes on beyond the tile's first or last record becomes a record
//             (entry, partial sum) of the next array, which has two slots per tile: slot 2t for the fragment that crosses tile t's left
//             edge, slot 2t + 1 for the one that crosses its right edge.  A fragment that crosses both fills slot 2t, and slot 2t + 1
//             repeats the entry with the ABSENT mark (it keeps the run contiguous and is skipped by the sum); a slot without a fragment is
//             NONE.  The same step runs on that array, and on the next, until an array fits one tile: ceil-log-many launches whose number
//             and sizes follow from n alone, so the call reads nothing back and can be captured in a graph.
// The contribution of a record is recomputed from its slot with the code of the atomic paths: corner_weight after locate (grid_index.h),
// corner_terms<double, D, false> after locate_d2 (grid_second.h; from the fp32 phi, 1 - phi and phi', rounded to fp32 once), one fp32 product
// with the gradient value.
#include "common.h"
#include "grid_index.h"
#include "grid_second.h"
#include <math.h>

namespace ngp {

constexpr int ORD_THREADS = 256;
constexpr uint32_t ORD_TILE = 64;              // records per tile of the sum = lanes of a wave
constexpr uint32_t ORD_NONE = 0xffffffffu;     // no record (an empty slot, a record of a point outside the level)
constexpr uint32_t ORD_ABSENT = 0x80000000u;   // the record repeats its left neighbour's entry and carries no value
constexpr uint32_t ORD_RADIX_TILE = 256;       // items per scatter step = threads of the histogram / scatter workgroups
constexpr uint32_t ORD_MAX_GROUPS = 1024;      // workgroups per radix pass (each owns a contiguous range of tiles)
constexpr uint32_t ORD_COUNT_WORDS = 256 * ORD_MAX_GROUPS + 256;   // per-(digit, group) counts, then the 256 digit totals
constexpr uint32_t ORD_RADIX_PASSES = 4;       // launched; a level works in radix_digits(level_size) of them
constexpr int ORD_MAX_ARRAYS = 8;              // arrays of partial sums: 5 for the largest call (2^31 records)

__device__ __forceinline__ uint32_t level_size_of(const int32_t* __restrict__ offsets, uint32_t level) {
    return (uint32_t)offsets[level + 1] - (uint32_t)offsets[level];
}
// 8-bit digits of the largest key, level_size itself
__device__ __forceinline__ uint32_t radix_digits(uint32_t level_size) { return (32u - (uint32_t)__builtin_clz(level_size | 1u) + 7u) >> 3; }

// ------------------------------------------------------------------------------------------------
// records and sort
// ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(ORD_THREADS) void k_ord_records(const float* __restrict__ inputs, const int32_t* __restrict__ offsets, uint32_t B,
                                                             uint32_t level, float scale, uint32_t resolution, uint32_t gridtype, bool align_corners,
                                                             uint32_t interp, InputMap im, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t level_size = level_size_of(offsets, level);
    LevelIndexer<D> indexer;
    indexer.init(gridtype, align_corners, level_size, resolution);
    for (uint32_t b = blockIdx.x * ORD_THREADS + threadIdx.x; b < B; b += gridDim.x * ORD_THREADS) {
        float frac[D], deriv[D];
        uint32_t cell[D];
        const bool inside = locate<D>(inputs + (size_t)b * D, scale, align_corners, interp, frac, deriv, cell, im);
        constexpr int UK = D == 5 ? 8 : (1 << D);   // (32 corners unrolled spill SGPRs in the debug-bounds build)
#pragma unroll UK
        for (int k = 0; k < (1 << D); k++) {
            uint32_t pg[D];
#pragma unroll
            for (int d = 0; d < D; d++) pg[d] = cell[d] + ((k >> d) & 1);
            const uint32_t slot = (b << D) | (uint32_t)k;
            const uint32_t idx = inside ? indexer(pg) : level_size;
            NGP_BOUNDS(idx <= level_size);
            keys[slot] = idx;
            vals[slot] = slot;
        }
    }
}

// digit counts of one workgroup's range: hist[digit * groups + group]
__global__ __launch_bounds__(ORD_RADIX_TILE) void k_ord_radix_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t pass, uint32_t tiles_per_group,
                                                                   uint32_t groups, const int32_t* __restrict__ offsets, uint32_t level,
                                                                   uint32_t* __restrict__ hist) {
    if (pass >= radix_digits(level_size_of(offsets, level))) return;
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t shift = 8u * pass;
    const uint32_t begin = blockIdx.x * tiles_per_group * ORD_RADIX_TILE;
    const uint32_t end = min(n, begin + tiles_per_group * ORD_RADIX_TILE);
    for (uint32_t i = begin + threadIdx.x; i < end; i += ORD_RADIX_TILE) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[threadIdx.x * groups + blockIdx.x] = h[threadIdx.x];
}

// one workgroup per digit: exclusive scan of the digit's group counts in place, the digit's total to totals[digit]
__global__ __launch_bounds__(ORD_MAX_GROUPS) void k_ord_radix_scan(uint32_t* __restrict__ hist, uint32_t groups, uint32_t pass,
                                                                   const int32_t* __restrict__ offsets, uint32_t level, uint32_t* __restrict__ totals) {
    if (pass >= radix_digits(level_size_of(offsets, level))) return;
    __shared__ uint32_t part[ORD_MAX_GROUPS];
    const uint32_t t = threadIdx.x, digit = blockIdx.x;
    const uint32_t v = t < groups ? hist[digit * groups + t] : 0u;
    part[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < ORD_MAX_GROUPS; o <<= 1) {
        const uint32_t a = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += a;
        __syncthreads();
    }
    if (t < groups) hist[digit * groups + t] = part[t] - v;
    if (t == ORD_MAX_GROUPS - 1) totals[digit] = part[t];
}

// stable scatter: a workgroup walks its range tile by tile in order; inside a tile an item's rank among the earlier items with its digit
// comes from the lanes of its wave (8 ballots -> the lanes with the same digit, mbcnt) and the counts of the earlier waves.  A digit's first
// slot for this workgroup: the totals of the smaller digits (scanned here, by every workgroup) + its scanned group count
__global__ __launch_bounds__(ORD_RADIX_TILE) void k_ord_radix_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t n,
                                                                      uint32_t pass, uint32_t tiles_per_group, uint32_t groups,
                                                                      const int32_t* __restrict__ offsets, uint32_t level,
                                                                      const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals,
                                                                      uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    if (pass >= radix_digits(level_size_of(offsets, level))) return;
    constexpr uint32_t WAVES = ORD_RADIX_TILE / 64;
    __shared__ uint32_t run[256];
    __shared__ uint32_t wave_count[WAVES][256];
    const uint32_t t = threadIdx.x, wave = t >> 6, shift = 8u * pass;
    run[t] = totals[t];
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t a = t >= o ? run[t - o] : 0u;
        __syncthreads();
        run[t] += a;
        __syncthreads();
    }
    run[t] += hist[t * groups + blockIdx.x] - totals[t];
    const uint32_t begin = blockIdx.x * tiles_per_group * ORD_RADIX_TILE;
    const uint32_t end = min(n, begin + tiles_per_group * ORD_RADIX_TILE);
    for (uint32_t base = begin; base < end; base += ORD_RADIX_TILE) {
        const uint32_t i = base + t;
        const bool valid = i < end;
        uint32_t key = 0u, val = 0u, digit = 0u;
        if (valid) {
            key = keys_in[i];
            val = vals_in[i];
            digit = (key >> shift) & 255u;
        }
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (digit >> bit) & 1u;
            const uint64_t m = __ballot(valid && set);
            same &= set ? m : ~m;
        }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) wave_count[w][t] = 0u;
        __syncthreads();
        if (valid && rank == 0u) wave_count[wave][digit] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[digit] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += wave_count[w][digit];
            NGP_BOUNDS(pos < n);
            keys_out[pos] = key;
            vals_out[pos] = val;
        }
        __syncthreads();
        uint32_t add = 0u;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) add += wave_count[w][t];
        run[t] += add;
        __syncthreads();
    }
}

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
    const bool odd = radix_digits(level_size) & 1u;   // where the last working radix pass left the records
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
        float w;
        if constexpr (ORDER == 1) {
            float frac[D], deriv[D];
            uint32_t cell[D];
            locate<D>(inputs + (size_t)b * D, scale, align_corners, interp, frac, deriv, cell, im);
            w = corner_weight<D>(frac, k);
        } else {
            // a_k from the fp32 phi, 1 - phi and phi' in double, rounded once: the sum over d of terms of both signs cancels, and the fp32
            // form of the atomic path is exact only relative to the terms, not to a_k (the bound of the tests is relative to |a_k g|)
            float phi[D], d1[D], d2[D];
            double u[D], unused[D];
            uint32_t cell[D];
            locate_d2<D>(inputs + (size_t)b * D, scale, align_corners, interp, phi, d1, d2, cell);
#pragma unroll
            for (int d = 0; d < D; d++) u[d] = (double)uin[(size_t)b * D + d];
            w = (float)corner_terms<double, D, false>(phi, d1, d2, u, k, (double)scale, unused);
        }
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
static size_t align256(uint64_t bytes) { return (size_t)((bytes + 255u) & ~(uint64_t)255u); }

// the workspace of a call: a function of (B, D, C) alone.  Keys / values twice (ping-pong) for the n = B << D records of one level, the
// radix counts, then the arrays of partial sums: m_1 = 2 ceil(n / 64) records, m_2 = 2 ceil(m_1 / 64), ... until one fits a tile
struct OrdLayout {
    size_t keys[2], vals[2], hist, total;
    uint32_t n, n_arrays;               // arrays of partial sums (the sum launches are n_arrays + 1)
    uint32_t m[ORD_MAX_ARRAYS];
    size_t part_keys[ORD_MAX_ARRAYS], part_vals[ORD_MAX_ARRAYS];
};

static OrdLayout ord_layout(uint32_t B, uint32_t D, uint32_t C) {
    OrdLayout w = {};
    w.n = B << D;   // (B << D <= 2^31: checked by the callers)
    const size_t a = align256((uint64_t)w.n * sizeof(uint32_t));
    w.keys[0] = 0; w.vals[0] = a; w.keys[1] = 2 * a; w.vals[1] = 3 * a; w.hist = 4 * a;
    size_t at = 4 * a + align256(ORD_COUNT_WORDS * sizeof(uint32_t));
    for (uint32_t m = w.n; m > ORD_TILE; w.n_arrays++) {
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
    uint32_t* keys[2] = {(uint32_t*)(ws + w.keys[0]), (uint32_t*)(ws + w.keys[1])};
    uint32_t* vals[2] = {(uint32_t*)(ws + w.vals[0]), (uint32_t*)(ws + w.vals[1])};
    uint32_t* hist = (uint32_t*)(ws + w.hist);
    uint32_t* totals = hist + 256 * ORD_MAX_GROUPS;
    const uint32_t n = w.n;
    const uint32_t tiles = cdiv(n, ORD_RADIX_TILE);
    const uint32_t tiles_per_group = cdiv(tiles, ORD_MAX_GROUPS);
    const uint32_t groups = cdiv(tiles, tiles_per_group);
    auto part_keys = [&](uint32_t i) { return i < w.n_arrays ? (uint32_t*)(ws + w.part_keys[i]) : nullptr; };
    auto part_vals = [&](uint32_t i) { return i < w.n_arrays ? (float*)(ws + w.part_vals[i]) : nullptr; };
    for (uint32_t level = 0; level < a.L; level++) {
        NGP_LAUNCH((k_ord_records<D>), dim3(grid_blocks(a.B, ORD_THREADS)), dim3(ORD_THREADS), 0, st, a.inputs, a.offsets, a.B, level,
                           a.lv.scale[level], a.lv.res[level], a.gridtype, a.align_corners, a.interp, a.im, keys[0], vals[0]);
        for (uint32_t pass = 0; pass < ORD_RADIX_PASSES; pass++) {
            const uint32_t src = pass & 1u;
            NGP_LAUNCH(k_ord_radix_hist, dim3(groups), dim3(ORD_RADIX_TILE), 0, st, keys[src], n, pass, tiles_per_group, groups, a.offsets, level,
                               hist);
            NGP_LAUNCH(k_ord_radix_scan, dim3(256), dim3(ORD_MAX_GROUPS), 0, st, hist, groups, pass, a.offsets, level, totals);
            NGP_LAUNCH(k_ord_radix_scatter, dim3(groups), dim3(ORD_RADIX_TILE), 0, st, keys[src], vals[src], n, pass, tiles_per_group, groups,
                               a.offsets, level, hist, totals, keys[src ^ 1u], vals[src ^ 1u]);
        }
        // one wave per tile of 64 records, the exact grid (the order does not depend on it: a tile is a fixed slice of the array)
        NGP_LAUNCH((k_ord_sum_records<T, D, C, ORDER>), dim3((uint32_t)cdiv64((uint64_t)cdiv(n, ORD_TILE) * ORD_TILE, ORD_THREADS)),
                           dim3(ORD_THREADS), 0, st, keys[0], vals[0], keys[1], vals[1], n, (const T*)a.grad, a.inputs, (const T*)a.u, a.offsets,
                           (T*)a.grad_embeddings, a.B, level, a.lv.scale[level], a.align_corners, a.interp, a.im, part_keys(0), part_vals(0));
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

static int check_ordered_workspace(const char* fn, uint32_t B, uint32_t D, uint32_t C, int dtype, const void* workspace, size_t workspace_bytes) {
    NGP_REQUIRE(((uint64_t)B << D) <= (1ull << 31), NGP_ERR_INVALID, "%s: B * 2^D must not exceed 2^31 (B=%u, D=%u)", fn, B, D);
    const size_t need = ngp_grid_ordered_workspace_bytes(B, D, C, dtype);
    NGP_REQUIRE(workspace && workspace_bytes >= need, NGP_ERR_INVALID, "%s: needs a workspace of %zu bytes (ngp_grid_ordered_workspace_bytes), got %zu",
                fn, need, workspace ? workspace_bytes : (size_t)0);
    NGP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, NGP_ERR_INVALID, "%s: workspace must be 256-byte aligned", fn);
    return NGP_OK;
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
    OrdArgs a = {};
    a.grad = grad;
    a.inputs = inputs;
    a.offsets = offsets;
    a.grad_embeddings = grad_embeddings;
    a.B = B;
    a.L = L;
    a.gridtype = gridtype;
    a.interp = interp;
    a.align_corners = align_corners != 0;
    a.im = InputMap{0.0f, 0.0f};
    if (bound > 0.0f) a.im = InputMap{bound, 1.0f / (float)(2.0 * (double)bound)};   // (gridencoder.hip: make_input_map)
    a.workspace = workspace;
    fill_levels(a.lv, L, S, H);
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
    OrdArgs a = {};
    a.grad = grad;
    a.inputs = inputs;
    a.offsets = offsets;
    a.u = grad_grad_inputs;
    a.grad_embeddings = grad_embeddings;
    a.B = B;
    a.L = L;
    a.gridtype = gridtype;
    a.interp = interp;
    a.align_corners = align_corners != 0;
    a.im = InputMap{0.0f, 0.0f};
    a.workspace = workspace;
    fill_levels(a.lv, L, S, H);
    const hipStream_t st = as_stream(stream);
    return dtype == NGP_F16 ? dispatch_ordered_second<half_t>(D, C, a, embeddings, grad_grad, grad_inputs2, st)
                            : dispatch_ordered_second<float>(D, C, a, embeddings, grad_grad, grad_inputs2, st);
}
