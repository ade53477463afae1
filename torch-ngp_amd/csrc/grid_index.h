// Grid-encoder indexing shared by the fp16/fp32 kernels (gridencoder.hip), the fp64 ones (fp64.hip), the second-order backward
// (grid_second.hip), the record sort (grid_records.hip) and the ordered scatter (grid_ordered.hip): the per-level table, the corner-index
// rule, the position of a point inside a level and its input map, the corner weight and the first backward's input term.  One statement of each, so the fp64 path locates points and computes
// interpolation weights exactly as the fp32 path does.  Also the host plumbing the units share: the level table of a call, the launch-grid
// cap and the (D, C) dispatch.
#pragma once
#include "common.h"

namespace ngp {

struct GridLevels {
    float scale[NGP_MAX_LEVELS];
    uint32_t res[NGP_MAX_LEVELS];
};

// host: the per-level scale / resolution table of a call (ngp_grid_level_table: the reproducible recipe shared with the oracle)
inline void fill_levels(GridLevels& lv, uint32_t L, float S, uint32_t H) { ngp_grid_level_table(L, S, H, lv.scale, lv.res); }

// host: workgroups of a grid-stride launch over n items, capped so that a (blocks, level) grid stays level-major
inline uint32_t grid_blocks(uint64_t n, uint32_t threads) {
    const uint64_t nb = cdiv64(n, threads);
    return nb < 1 ? 1u : (nb > 65535u ? 65535u : (uint32_t)nb);
}

// host: `return <expression>;` with the run-time pair (D, C) as the compile-time constants D_, C_ of the expression; falls through for a
// pair outside D in [2, 5], C in {1, 2, 4, 8}
#define NGP_DC_CASE_(DD, CC, ...) \
    case DD * 16 + CC: {          \
        constexpr int D_ = DD, C_ = CC; \
        return __VA_ARGS__;       \
    }
#define NGP_DC_ROW_(DD, ...) NGP_DC_CASE_(DD, 1, __VA_ARGS__) NGP_DC_CASE_(DD, 2, __VA_ARGS__) NGP_DC_CASE_(DD, 4, __VA_ARGS__) NGP_DC_CASE_(DD, 8, __VA_ARGS__)
#define NGP_DISPATCH_DC(D, C, ...)                                                                                                  \
    switch ((D) * 16 + (C)) {                                                                                                       \
        NGP_DC_ROW_(2, __VA_ARGS__) NGP_DC_ROW_(3, __VA_ARGS__) NGP_DC_ROW_(4, __VA_ARGS__) NGP_DC_ROW_(5, __VA_ARGS__)             \
        default: break;                                                                                                             \
    }

__constant__ const uint32_t kPrimes[7] = {1u, 2654435761u, 805459861u, 3674653429u,
                                          2097192037u, 1434869437u, 2165219737u};

// Wave-uniform description of how a level is indexed (gridencoder.cu:66-84, get_grid_index).
template <int D>
struct LevelIndexer {
    uint32_t stride[D];  // dense strides of the dims that take part (0 for the others)
    uint32_t size;       // hashmap_size
    uint32_t mask;       // size-1 if size is a power of two else 0
    bool hashed;
    bool need_mod;       // false when a dense index is provably < size

    __host__ __device__ __forceinline__ void init(uint32_t gridtype, bool align_corners, uint32_t hashmap_size,
                                                  uint32_t resolution) {
        uint32_t s = 1;
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (s <= hashmap_size) {
                stride[d] = s;
                s *= align_corners ? resolution : (resolution + 1u);
            } else {
                stride[d] = 0;
            }
        }
        hashed = (gridtype == 0u) && (s > hashmap_size);
        // without align_corners every corner coordinate is <= resolution and the strides are powers of (resolution + 1):
        // a dense index over all D dims is < (resolution+1)^D <= size.  With align_corners the stride base is
        // `resolution` while a corner can sit AT `resolution`, so the index can wrap (gridencoder.cu:66-84).
        need_mod = hashed || (s > hashmap_size) || align_corners;
        size = hashmap_size;
        mask = ((hashmap_size & (hashmap_size - 1u)) == 0u) ? hashmap_size - 1u : 0u;
    }

    // The same index from per-dimension terms: term(d, c) for the lower vertex coordinate c, step(d) to get the upper one
    // ((c + 1) * k == c * k + k in uint32 arithmetic), combine() over one term per dimension.  A cell's 2^D corners then cost D
    // multiplications instead of D * 2^D (v_mul_lo_u32 is a quarter-rate instruction).
    __device__ __forceinline__ uint32_t term(int d, uint32_t c) const { return hashed ? c * kPrimes[d] : c * stride[d]; }
    __device__ __forceinline__ uint32_t step(int d) const { return hashed ? kPrimes[d] : stride[d]; }
    __device__ __forceinline__ uint32_t combine(const uint32_t (&t)[D]) const {
        uint32_t idx = 0;
        if (hashed) {
#pragma unroll
            for (int d = 0; d < D; d++) idx ^= t[d];
        } else {
#pragma unroll
            for (int d = 0; d < D; d++) idx += t[d];
        }
        if (!need_mod) return idx;
        return mask ? (idx & mask) : (idx % size);
    }

    __device__ __forceinline__ uint32_t operator()(const uint32_t (&pg)[D]) const {
        uint32_t idx = 0;
        if (hashed) {
#pragma unroll
            for (int d = 0; d < D; d++) idx ^= pg[d] * kPrimes[d];
        } else {
#pragma unroll
            for (int d = 0; d < D; d++) idx += pg[d] * stride[d];
        }
        if (!need_mod) return idx;
        return mask ? (idx & mask) : (idx % size);
    }
};

// gridencoder.cu:146-159: position inside the level.  Returns false when the point is outside [0,1]^D.
// Input mapping of the fused path: the module maps [-bound, bound] -> [0, 1] as (x + bound) * (1 / (2 bound)) in fp32
// (grid.py:149 through PyTorch's scalar-division kernel); InputMap{shift = bound, scale = 1/(2 bound)} reproduces those two
// roundings inside the kernel, scale == 0 means the inputs already are unit coordinates (the reference op contract).
struct InputMap {
    float shift, scale;
};
// host: the map of a call's `bound` (<= 0: unit coordinates)
inline InputMap make_input_map(float bound) {
    InputMap im{0.0f, 0.0f};
    if (bound > 0.0f) {
        im.shift = bound;
        im.scale = 1.0f / (float)(2.0 * (double)bound);
    }
    return im;
}

// entries idx and idx + 1 of an fp16 C = 2 table -- the two corners of a dense level that differ in the first coordinate -- in one 8-byte
// load (4-byte aligned: global_load_dwordx2); .x = entry idx, .y = entry idx + 1, each a half2
__device__ __forceinline__ uint2 load_x_pair(const _Float16* __restrict__ table, uint32_t idx) {
    uint2 q;
    __builtin_memcpy(&q, table + (size_t)idx * 2, sizeof(uint2));
    return q;
}

template <int D>
__device__ __forceinline__ bool locate(const float* __restrict__ x, float scale, bool align_corners, uint32_t interp,
                                       float (&frac)[D], float (&deriv)[D], uint32_t (&cell)[D], InputMap im = InputMap{0.0f, 0.0f}) {
    float xv[D];
    bool inside = true;
#pragma unroll
    for (int d = 0; d < D; d++) {
        xv[d] = x[d];
        if (im.scale != 0.0f) xv[d] = (xv[d] + im.shift) * im.scale;
        inside = inside && !(xv[d] < 0.0f || xv[d] > 1.0f);
    }
    if (!inside) return false;
#pragma unroll
    for (int d = 0; d < D; d++) {
        float p = __builtin_fmaf(xv[d], scale, align_corners ? 0.0f : 0.5f);
        float fl = floorf(p);
        cell[d] = (uint32_t)fl;
        p -= (float)cell[d];
        if (interp == 1u) {
            deriv[d] = 6.0f * p * (1.0f - p);
            p = p * p * (3.0f - 2.0f * p);
        } else {
            deriv[d] = 1.0f;
        }
        frac[d] = p;
    }
    return true;
}

// locate() for the second-order backward (grid_second.hip): the same position, cell, phi and phi', plus phi'' of the raw fraction
// (0 for linear interpolation, 6 - 12 f for smoothstep).  Unit inputs only (no InputMap).
template <int D>
__device__ __forceinline__ bool locate_d2(const float* __restrict__ x, float scale, bool align_corners, uint32_t interp, float (&frac)[D],
                                          float (&deriv)[D], float (&deriv2)[D], uint32_t (&cell)[D]) {
    float xv[D];
    bool inside = true;
#pragma unroll
    for (int d = 0; d < D; d++) {
        xv[d] = x[d];
        inside = inside && !(xv[d] < 0.0f || xv[d] > 1.0f);
    }
    if (!inside) return false;
#pragma unroll
    for (int d = 0; d < D; d++) {
        float p = __builtin_fmaf(xv[d], scale, align_corners ? 0.0f : 0.5f);
        float fl = floorf(p);
        cell[d] = (uint32_t)fl;
        p -= (float)cell[d];
        if (interp == 1u) {
            deriv[d] = 6.0f * p * (1.0f - p);
            deriv2[d] = 6.0f - 12.0f * p;
            p = p * p * (3.0f - 2.0f * p);
        } else {
            deriv[d] = 1.0f;
            deriv2[d] = 0.0f;
        }
        frac[d] = p;
    }
    return true;
}

// interpolation weight of corner k (bit d set: the upper vertex in dimension d) -- the fp32 product of k_grid_forward, same order
template <int D>
__device__ __forceinline__ float corner_weight(const float (&frac)[D], uint32_t k) {
    float w = 1.0f;
#pragma unroll
    for (int d = 0; d < D; d++) w *= ((k >> d) & 1u) ? frac[d] : (1.0f - frac[d]);
    return w;
}

// gridencoder.cu:343-369: grad_inputs[b, d] = sum_{l, c} grad[l, b, c] * dy_dx[b, l, d, c] -- one statement for the first-order backward
// (gridencoder.hip) and its ordered form (grid_ordered.hip): the same bits from both
template <typename T>
__global__ void k_grid_input_backward(const T* __restrict__ grad, const T* __restrict__ dy_dx, T* __restrict__ grad_inputs,
                                      uint32_t B, uint32_t L, uint32_t D, uint32_t C) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    const T* dd = dy_dx + (size_t)b * L * D * C;
    float r = 0.0f;
    for (uint32_t l = 0; l < L; l++)
        for (uint32_t c = 0; c < C; c++)
            r = __builtin_fmaf((float)grad[((size_t)l * B + b) * C + c], (float)dd[(l * D + d) * C + c], r);
    grad_inputs[t] = (T)r;
}

}  // namespace ngp
