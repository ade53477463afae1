// The record sort of the grid encoder's bit-reproducible table gradients (grid_records.hip): one record per (point, corner)
// of a level, sorted by table entry with a stable LSD radix sort.  Shared by the fp64 backwards (fp64.hip, first and second order) and the
// ordered fp32 / fp16 scatter (grid_ordered.hip), which differ only in how they sum an entry's run.
//   record    n = B << D of them: key = the entry inside the level (level_size for a point outside [0,1]^D: sorts after every entry,
//             contributes nothing), value = the slot b << D | k.  A consumer skips every key >= level_size;
//   sort      8 bits a pass.  Four passes are launched (the host does not know the level sizes: the offsets are device memory, and nothing is
//             read back), a pass above bit_length(level_size) returns at once.  The sorted records are in side rec_sorted_side(level_size)
//             of the ping-pong buffers.  The sorted order is a function of the keys alone: equal keys keep slot order.
#pragma once
#include "common.h"
#include "grid_index.h"

namespace ngp {

constexpr int REC_THREADS = 256;               // threads of the record kernel
constexpr uint32_t REC_RADIX_TILE = 256;       // items per scatter step = threads of the histogram / scatter workgroups
constexpr uint32_t REC_MAX_GROUPS = 1024;      // workgroups per radix pass (each owns a contiguous range of tiles)
constexpr uint32_t REC_COUNT_WORDS = 256 * REC_MAX_GROUPS + 256;   // per-(digit, group) counts, then the 256 digit totals
constexpr uint32_t REC_RADIX_PASSES = 4;       // launched; a level works in radix_digits(level_size) of them

__device__ __forceinline__ uint32_t level_size_of(const int32_t* __restrict__ offsets, uint32_t level) {
    return (uint32_t)offsets[level + 1] - (uint32_t)offsets[level];
}
// 8-bit digits of the largest key, level_size itself
__device__ __forceinline__ uint32_t radix_digits(uint32_t level_size) { return (32u - (uint32_t)__builtin_clz(level_size | 1u) + 7u) >> 3; }
// the ping-pong side (0 / 1) in which the last working radix pass left the records
__device__ __forceinline__ uint32_t rec_sorted_side(uint32_t level_size) { return radix_digits(level_size) & 1u; }

// host: the sort's part of a workspace, a function of (B, D) alone.  Byte offsets of the keys / values (ping-pong) of the n = B << D records
// of one level and of the radix counts; `bytes`: their total, where a caller's own arrays may follow (a multiple of 256)
struct RecLayout {
    uint32_t n;
    size_t keys[2], vals[2], counts, bytes;
};
inline size_t align256(uint64_t bytes) { return (size_t)((bytes + 255u) & ~(uint64_t)255u); }
inline RecLayout rec_layout(uint32_t B, uint32_t D) {
    RecLayout w = {};
    w.n = B << D;   // (B << D <= 2^31: rec_check_workspace)
    const size_t a = align256((uint64_t)w.n * sizeof(uint32_t));
    w.keys[0] = 0; w.vals[0] = a; w.keys[1] = 2 * a; w.vals[1] = 3 * a; w.counts = 4 * a;
    w.bytes = 4 * a + align256(REC_COUNT_WORDS * sizeof(uint32_t));
    return w;
}

// host: both sides of the sorted records of a workspace (the kernels pick theirs with rec_sorted_side)
struct RecSides {
    const uint32_t *keys[2], *vals[2];
    uint32_t n;
};

// host: the record limit B * 2^D <= 2^31, the workspace's size (`need` bytes, the answer of the query named `query`) and its alignment.
// `prefix`: "fp64" for the fp64 branch of an entry that serves other dtypes without a workspace, "" otherwise
int rec_check_workspace(const char* fn, const char* prefix, const char* query, uint32_t B, uint32_t D, size_t need, const void* workspace,
                        size_t workspace_bytes);

// host: the records of one level, sorted, in `workspace` (rec_layout; checked by rec_check_workspace).  D in [2, 5]; `im`: the input map
// of the call (InputMap{0, 0}: unit coordinates).  Launches only: the caller's check_launch follows
RecSides rec_sort_level(uint32_t D, const float* inputs, const int32_t* offsets, uint32_t B, uint32_t level, float scale, uint32_t resolution,
                        uint32_t gridtype, bool align_corners, uint32_t interp, InputMap im, void* workspace, hipStream_t st);

}  // namespace ngp
