// The record sort of the grid encoder's bit-reproducible table gradients for gfx950 (MI355X): the record kernel, the three kernels of a
// radix pass and the host function that sorts one level (grid_records.h).  Compiled once, used by fp64.hip and
// grid_ordered.hip.
#include "grid_records.h"

namespace ngp {

template <int D>
__global__ __launch_bounds__(REC_THREADS) void k_rec_records(const float* __restrict__ inputs, const int32_t* __restrict__ offsets, uint32_t B,
                                                             uint32_t level, float scale, uint32_t resolution, uint32_t gridtype, bool align_corners,
                                                             uint32_t interp, InputMap im, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t level_size = level_size_of(offsets, level);
    LevelIndexer<D> indexer;
    indexer.init(gridtype, align_corners, level_size, resolution);
    for (uint32_t b = blockIdx.x * REC_THREADS + threadIdx.x; b < B; b += gridDim.x * REC_THREADS) {
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
__global__ __launch_bounds__(REC_RADIX_TILE) void k_rec_radix_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t pass, uint32_t tiles_per_group,
                                                                   uint32_t groups, const int32_t* __restrict__ offsets, uint32_t level,
                                                                   uint32_t* __restrict__ hist) {
    if (pass >= radix_digits(level_size_of(offsets, level))) return;
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t shift = 8u * pass;
    const uint32_t begin = blockIdx.x * tiles_per_group * REC_RADIX_TILE;
    const uint32_t end = min(n, begin + tiles_per_group * REC_RADIX_TILE);
    for (uint32_t i = begin + threadIdx.x; i < end; i += REC_RADIX_TILE) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[threadIdx.x * groups + blockIdx.x] = h[threadIdx.x];
}

// one workgroup per digit: exclusive scan of the digit's group counts in place, the digit's total to totals[digit]
__global__ __launch_bounds__(REC_MAX_GROUPS) void k_rec_radix_scan(uint32_t* __restrict__ hist, uint32_t groups, uint32_t pass,
                                                                   const int32_t* __restrict__ offsets, uint32_t level, uint32_t* __restrict__ totals) {
    if (pass >= radix_digits(level_size_of(offsets, level))) return;
    __shared__ uint32_t part[REC_MAX_GROUPS];
    const uint32_t t = threadIdx.x, digit = blockIdx.x;
    const uint32_t v = t < groups ? hist[digit * groups + t] : 0u;
    part[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < REC_MAX_GROUPS; o <<= 1) {
        const uint32_t a = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += a;
        __syncthreads();
    }
    if (t < groups) hist[digit * groups + t] = part[t] - v;
    if (t == REC_MAX_GROUPS - 1) totals[digit] = part[t];
}

// stable scatter: a workgroup walks its range tile by tile in order; inside a tile an item's rank among the earlier items with its digit
// comes from the lanes of its wave (8 ballots -> the lanes with the same digit, mbcnt) and the counts of the earlier waves.  A digit's first
// slot for this workgroup: the totals of the smaller digits (scanned here, by every workgroup) + its scanned group count
__global__ __launch_bounds__(REC_RADIX_TILE) void k_rec_radix_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t n,
                                                                      uint32_t pass, uint32_t tiles_per_group, uint32_t groups,
                                                                      const int32_t* __restrict__ offsets, uint32_t level,
                                                                      const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals,
                                                                      uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    if (pass >= radix_digits(level_size_of(offsets, level))) return;
    constexpr uint32_t WAVES = REC_RADIX_TILE / 64;
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
    const uint32_t begin = blockIdx.x * tiles_per_group * REC_RADIX_TILE;
    const uint32_t end = min(n, begin + tiles_per_group * REC_RADIX_TILE);
    for (uint32_t base = begin; base < end; base += REC_RADIX_TILE) {
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
// host
// ------------------------------------------------------------------------------------------------
int rec_check_workspace(const char* fn, const char* prefix, const char* query, uint32_t B, uint32_t D, size_t need, const void* workspace,
                        size_t workspace_bytes) {
    const bool named = prefix[0] != '\0';
    NGP_REQUIRE(((uint64_t)B << D) <= (1ull << 31), NGP_ERR_INVALID, "%s: %s%sB * 2^D must not exceed 2^31 (B=%u, D=%u)", fn, prefix, named ? ": " : "",
                B, D);
    NGP_REQUIRE(workspace && workspace_bytes >= need, NGP_ERR_INVALID, "%s: %s%sneeds a workspace of %zu bytes (%s), got %zu", fn, prefix,
                named ? " " : "", need, query, workspace ? workspace_bytes : (size_t)0);
    NGP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, NGP_ERR_INVALID, "%s: %s%sworkspace must be 256-byte aligned", fn, prefix,
                named ? ": " : "");
    return NGP_OK;
}

RecSides rec_sort_level(uint32_t D, const float* inputs, const int32_t* offsets, uint32_t B, uint32_t level, float scale, uint32_t resolution,
                        uint32_t gridtype, bool align_corners, uint32_t interp, InputMap im, void* workspace, hipStream_t st) {
    const RecLayout w = rec_layout(B, D);
    char* ws = (char*)workspace;
    uint32_t* keys[2] = {(uint32_t*)(ws + w.keys[0]), (uint32_t*)(ws + w.keys[1])};
    uint32_t* vals[2] = {(uint32_t*)(ws + w.vals[0]), (uint32_t*)(ws + w.vals[1])};
    uint32_t* hist = (uint32_t*)(ws + w.counts);
    uint32_t* totals = hist + 256 * REC_MAX_GROUPS;
    const uint32_t n = w.n;
    const uint32_t tiles = cdiv(n, REC_RADIX_TILE);
    const uint32_t tiles_per_group = cdiv(tiles, REC_MAX_GROUPS);
    const uint32_t groups = cdiv(tiles, tiles_per_group);
#define REC_RECORDS_(DD)                                                                                                                       \
    NGP_LAUNCH((k_rec_records<DD>), dim3(grid_blocks(B, REC_THREADS)), dim3(REC_THREADS), 0, st, inputs, offsets, B, level, scale, resolution, \
               gridtype, align_corners, interp, im, keys[0], vals[0])
    switch (D) {
        case 2: REC_RECORDS_(2); break;
        case 3: REC_RECORDS_(3); break;
        case 4: REC_RECORDS_(4); break;
        default: REC_RECORDS_(5); break;
    }
#undef REC_RECORDS_
    for (uint32_t pass = 0; pass < REC_RADIX_PASSES; pass++) {
        const uint32_t src = pass & 1u;
        NGP_LAUNCH(k_rec_radix_hist, dim3(groups), dim3(REC_RADIX_TILE), 0, st, keys[src], n, pass, tiles_per_group, groups, offsets, level, hist);
        NGP_LAUNCH(k_rec_radix_scan, dim3(256), dim3(REC_MAX_GROUPS), 0, st, hist, groups, pass, offsets, level, totals);
        NGP_LAUNCH(k_rec_radix_scatter, dim3(groups), dim3(REC_RADIX_TILE), 0, st, keys[src], vals[src], n, pass, tiles_per_group, groups, offsets,
                           level, hist, totals, keys[src ^ 1u], vals[src ^ 1u]);
    }
    return RecSides{{keys[0], keys[1]}, {vals[0], vals[1]}, n};
}

}  // namespace ngp
