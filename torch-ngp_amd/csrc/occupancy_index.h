// Where a position falls in the occupancy bitfield: the Morton code, the clamp and the cascade exponent the marcher (raymarching.hip:
// probe_geom) and the culled extraction lattice (surface_nets.hip: k_lattice_*) both use -- ONE statement of each.
#pragma once
#include "common.h"
#include <math.h>

namespace ngp {

// raymarching.cu:56-81
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3D_1(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}

// clamp of a value to [lo, hi] with lo <= hi as ONE instruction (v_med3_f32).  `fminf(hi, fmaxf(lo, x))` is two, plus a v_max(x, x) per
// operand the compiler cannot prove quiet (IEEE mode) -- recomputed in every iteration of the march loop for the loop-invariant bounds too.
// Same result for every x incl. NaN (both forms return lo); NOT for lo > hi, which is why step_dt keeps the two-instruction form.
__device__ __forceinline__ float clamp_med3(float x, float lo, float hi) { return __builtin_amdgcn_fmed3f(x, lo, hi); }

__device__ __forceinline__ int mip_exponent(float mx, float Cm1) {
    int e;
    (void)frexpf(mx, &e);
    return (int)clamp_med3((float)e, 0.0f, Cm1);
}

}  // namespace ngp
