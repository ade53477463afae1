// The fp64 paths (fp64.hip) behind the dtype == NGP_F64 branches of the grid-encoder and SH entry points (gridencoder.hip,
// shencoder.hip).  Host functions; arguments are validated by the callers except where noted.
#pragma once
#include "common.h"

namespace ngp {

int f64_grid_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs, uint32_t B, uint32_t D, uint32_t C,
                     uint32_t L, float S, uint32_t H, void* dy_dx, uint32_t gridtype, bool align_corners, uint32_t interp, hipStream_t st);
// scratch of the deterministic backward: a function of B and D alone (the sort runs one level at a time), 0 for B == 0
size_t f64_grid_backward_workspace_bytes(uint32_t B, uint32_t D);
// checks the workspace size and the record limits itself
int f64_grid_backward(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                      uint32_t L, float S, uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype, bool align_corners, uint32_t interp,
                      void* workspace, size_t workspace_bytes, hipStream_t st);
// one level's records (table entry, point << D | corner) sorted by entry, stable, in the workspace of f64_grid_backward_workspace_bytes: the
// runs the first-order fp64 backward sums, for the second-order one (grid_second.hip).  D in [2, 5], B << D <= 2^31: checked by the callers
void f64_grid_sort_level(uint32_t D, const float* inputs, const int32_t* offsets, uint32_t B, uint32_t level, float scale, uint32_t resolution,
                         uint32_t gridtype, bool align_corners, uint32_t interp, void* workspace, const uint32_t** keys, const uint32_t** vals,
                         hipStream_t st);
int f64_grad_tv(const void* inputs, const void* embeddings, void* grad, const int32_t* offsets, float weight, uint32_t B, uint32_t D, uint32_t C,
                uint32_t L, float S, uint32_t H, uint32_t gridtype, bool align_corners, hipStream_t st);
int f64_sh_forward(const void* inputs, void* outputs, uint32_t B, uint32_t C, void* dy_dx, hipStream_t st);
int f64_sh_backward(const void* grad, uint32_t B, uint32_t C, const void* dy_dx, void* grad_inputs, hipStream_t st);

}  // namespace ngp
