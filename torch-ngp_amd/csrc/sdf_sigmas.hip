// Signed distances -> the density the compositors render: NeuS's section opacity (renderer.py: alpha = clip((prev_cdf -
// next_cdf + 1e-5) / (prev_cdf + 1e-5), 0, 1)) expressed as sigma = -log(1 - alpha) / deltas[:,0], the number every compositor of the library
// turns back into that alpha (raymarching.cu:501-577: alpha = 1 - exp(-sigma * deltas[:,0])).  One launch forward; one launch backward plus
// the one-workgroup pass that finishes grad_inv_s.  The kernel bodies and the host half live in sdf_sigmas.h, shared with the fp64 twins of
// fp64.hip; this unit holds the fp32 kernels, their entries and the workspace query.
#include "sdf_sigmas.h"

namespace ngp {
SDF_SIGMAS_KERNELS(float, k_sdf_sigmas)
static const SdfKernels<float> sdf_kernels_f32 = {k_sdf_sigmas_fwd, k_sdf_sigmas_bwd, k_sdf_sigmas_inv_s};
}  // namespace ngp

using namespace ngp;

extern "C" size_t ngp_sdf_sigmas_workspace_bytes(uint32_t M) { return sdf_sigmas_workspace_bytes(M); }

extern "C" int ngp_sdf_sigmas_forward(const float* sdf, const float* normals, const float* dirs, const float* deltas, const float* inv_s, uint32_t M,
                                      float cos_anneal, float* sigmas, ngp_stream_t stream) {
    return sdf_sigmas_forward<float>("sdf_sigmas_forward", sdf_kernels_f32, sdf, normals, dirs, deltas, inv_s, M, cos_anneal, sigmas, as_stream(stream));
}

extern "C" int ngp_sdf_sigmas_backward(const float* grad_sigmas, const float* sdf, const float* normals, const float* dirs, const float* deltas,
                                       const float* inv_s, uint32_t M, float cos_anneal, float* grad_sdf, float* grad_normals, float* grad_dirs,
                                       float* grad_inv_s, void* workspace, size_t workspace_bytes, ngp_stream_t stream) {
    return sdf_sigmas_backward<float>("sdf_sigmas_backward", sdf_kernels_f32, grad_sigmas, sdf, normals, dirs, deltas, inv_s, M, cos_anneal, grad_sdf,
                                      grad_normals, grad_dirs, grad_inv_s, workspace, workspace_bytes, as_stream(stream));
}
