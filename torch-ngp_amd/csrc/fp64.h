// The fp64 paths (fp64.hip) behind the dtype == NGP_F64 branches of the grid-encoder and SH entry points (gridencoder.hip,
// grid_second.hip, shencoder.hip).  Host functions; arguments are validated by the callers except where noted.
#pragma once
#include "common.h"

namespace ngp {

struct GridLevels;   // (grid_index.h)

int f64_grid_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs, uint32_t B, uint32_t D, uint32_t C,
                     uint32_t L, float S, uint32_t H, void* dy_dx, uint32_t gridtype, bool align_corners, uint32_t interp, hipStream_t st);
// scratch of the deterministic table gradients, first and second order: the record sort's (grid_records.h), a function of B and D alone
// (the sort runs one level at a time), 0 for B == 0
size_t f64_grid_backward_workspace_bytes(uint32_t B, uint32_t D);
// the record limit B * 2^D <= 2^31, the workspace's size and its alignment; `query`: the public query the message names
int f64_grid_check_workspace(const char* fn, const char* query, uint32_t B, uint32_t D, const void* workspace, size_t workspace_bytes);
// checks the workspace itself
int f64_grid_backward(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                      uint32_t L, float S, uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype, bool align_corners, uint32_t interp,
                      void* workspace, size_t workspace_bytes, hipStream_t st);
// grad_embeddings += the table gradient of every level, bit-reproducible.  order 1: sum w_k grad (the backward); order 2: sum a_k grad with
// u = dL2/dgx [B, D] (the backward's backward, grid_second.hip).  Workspace: checked by the caller (f64_grid_check_workspace)
int f64_grid_table_grad(uint32_t order, const void* grad, const float* inputs, const int32_t* offsets, const void* u, void* grad_embeddings,
                        uint32_t B, uint32_t D, uint32_t C, uint32_t L, const GridLevels& lv, uint32_t gridtype, bool align_corners, uint32_t interp,
                        void* workspace, hipStream_t st);
int f64_grad_tv(const void* inputs, const void* embeddings, void* grad, const int32_t* offsets, float weight, uint32_t B, uint32_t D, uint32_t C,
                uint32_t L, float S, uint32_t H, uint32_t gridtype, bool align_corners, hipStream_t st);
int f64_sh_forward(const void* inputs, void* outputs, uint32_t B, uint32_t C, void* dy_dx, hipStream_t st);
int f64_sh_backward(const void* grad, uint32_t B, uint32_t C, const void* dy_dx, void* grad_inputs, hipStream_t st);

}  // namespace ngp
