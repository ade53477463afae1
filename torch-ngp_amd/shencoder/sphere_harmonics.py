"""Spherical-harmonics direction encoder with the reference's surface (shencoder/sphere_harmonics.py:14-87):
`sh_encode(inputs, degree, calc_grad_inputs)`, `SHEncoder(input_dim=3, degree=4).forward(inputs, size=1)`.
Evaluated in fp32 (the reference forces it with custom_fwd(cast_inputs=float32)), float64 inputs in fp64.  The first backward is differentiable
(torch.autograd.grad(..., create_graph=True), eikonal / normal losses): DESIGN.md 3.8."""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

import _ngp_capi as _capi

try:  # the compiled binding first, as the reference does (shencoder/sphere_harmonics.py:8-11); the ctypes binding of the same C ABI otherwise
    import os as _os
    if _os.environ.get('NGP_HIP_LIBRARY'):  # a variant library is selected: the compiled module links the in-tree one, the ctypes binding follows the variable
        raise ImportError('NGP_HIP_LIBRARY is set')
    import _shencoder as _backend
except ImportError:
    from .backend import _backend


def _first_order_backward(grad, inputs, dy_dx, shape_info):
    n_points, dim, degree = shape_info
    grad_inputs = torch.zeros_like(inputs)
    _backend.sh_encode_backward(grad.contiguous(), inputs, n_points, dim, degree, dy_dx, grad_inputs)
    return grad_inputs


def sh_encode_backward_backward(grad, inputs, dy_dx, u, B, D, C, grad_grad, grad_inputs2):
    """ngp_sh_encode_backward_backward (include/ngp_hip.h) on tensors: grad [B,C*C], inputs [B,3], dy_dx [B,3*C*C], u [B,3]; grad_grad
    [B,C*C] and grad_inputs2 [B,3] overwritten (None: not computed).  All in the dtype of `inputs` (float32 or float64; float16 is
    refused by the entry)."""
    for t, name in ((grad, 'grad'), (inputs, 'inputs'), (dy_dx, 'dy_dx'), (u, 'grad_grad_inputs'), (grad_grad, 'grad_grad'),
                    (grad_inputs2, 'grad_inputs2')):
        if t is not None:
            _capi.dense(t, name)
            if t.dtype != inputs.dtype:
                raise RuntimeError(f"{name} must have the inputs' dtype {inputs.dtype} (got {t.dtype})")
    _capi.check(_capi.lib.ngp_sh_encode_backward_backward(_capi.ptr(grad), _capi.ptr(inputs), _capi.ptr(dy_dx), _capi.ptr(u), B, D, C,
                                                          _capi.ptr(grad_grad), _capi.ptr(grad_inputs2), _capi.float_code(inputs, 'inputs'),
                                                          _capi.stream()))


class _sh_encoder(Function):
    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, inputs, degree, calc_grad_inputs=False, caller=None):
        # the tensor of the graph: the caller's own (under autocast `inputs` is custom_fwd's fp32 copy of it).  A plain reference, not a
        # saved tensor: the first-order backward neither reads it nor checks its version
        ctx.source = inputs if caller is None else caller.tensor
        inputs = inputs.contiguous()
        n_points, dim = inputs.shape
        n_out = degree * degree
        outputs = torch.empty(n_points, n_out, dtype=inputs.dtype, device=inputs.device)
        dy_dx = torch.empty(n_points, dim * n_out, dtype=inputs.dtype, device=inputs.device) if calc_grad_inputs else None
        _backend.sh_encode_forward(inputs, outputs, n_points, dim, degree, dy_dx)
        ctx.save_for_backward(inputs, dy_dx)
        ctx.shape_info = (n_points, dim, degree)
        return outputs

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, grad):
        inputs, dy_dx = ctx.saved_tensors
        if dy_dx is None:  # directions did not require grad (the NeRF case)
            return None, None, None, None
        if torch.is_grad_enabled():
            # create_graph=True (eikonal / normal losses on d enc / d x): the same backend call as a differentiable op
            grad_inputs = _sh_backward.apply(grad, inputs.detach(), dy_dx, ctx.shape_info, ctx.source)
        else:
            grad_inputs = _first_order_backward(grad, inputs, dy_dx, ctx.shape_info)
        return grad_inputs, None, None, None


class _sh_backward(Function):
    """The first backward of the SH encoder as an op of its own, so that its result can be differentiated: forward is
    _first_order_backward, as _sh_encoder.backward (the same bits), backward is the second order (_sh_second).  `source` is
    the tensor the encoder was called with: dy_dx is a function of it, and d/d source is returned for it."""

    @staticmethod
    def forward(ctx, grad, inputs, dy_dx, shape_info, source):
        grad_inputs = _first_order_backward(grad, inputs, dy_dx, shape_info)
        ctx.save_for_backward(grad, inputs, dy_dx)
        ctx.shape_info = shape_info
        ctx.source = source
        ctx.set_materialize_grads(False)   # a result nobody differentiates reaches backward as None: nothing is launched
        return grad_inputs

    @staticmethod
    def backward(ctx, u):
        if u is None:
            return None, None, None, None, None
        grad, inputs, dy_dx = ctx.saved_tensors
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[4])
        d_grad, d_source = _sh_second.apply(u, grad, inputs, dy_dx, ctx.source, ctx.shape_info, needs)
        return d_grad, None, None, None, d_source


class _sh_second(Function):
    """Second order of the SH encoder: one call of ngp_sh_encode_backward_backward.  Its inputs include the upstream gradient and the
    directions the caller differentiates, so that differentiating its results once more reaches backward, which refuses third order."""

    @staticmethod
    def forward(ctx, u, grad, inputs, dy_dx, source, shape_info, needs):
        n_points, dim, degree = shape_info
        need_grad, need_source = needs
        d_grad = torch.empty(n_points, degree * degree, dtype=inputs.dtype, device=inputs.device) if need_grad else None
        d_source = torch.empty_like(inputs) if need_source else None
        if need_grad or need_source:
            sh_encode_backward_backward(grad.to(inputs.dtype).contiguous(), inputs, dy_dx, u.to(inputs.dtype).contiguous(), n_points, dim, degree,
                                        d_grad, d_source)
        if d_grad is not None:
            d_grad = d_grad.to(grad.dtype)
        if d_source is not None:
            d_source = d_source.to(dtype=source.dtype)   # an autocast caller's fp16 directions get an fp16 gradient
        return d_grad, d_source

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("sh_encode: third-order gradients are not provided (the SH encoder's second-order backward is not differentiable)")


def sh_encode(inputs, degree, calc_grad_inputs=False):
    return _sh_encoder.apply(inputs, degree, calc_grad_inputs, _capi.CallerTensor(inputs))


class SHEncoder(nn.Module):
    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        assert input_dim == 3, "SH encoder only support input dim == 3"
        assert 0 < degree <= 8, "SH encoder only supports degree in [1, 8]"
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = degree ** 2

    def __repr__(self):
        return f"SHEncoder: input_dim={self.input_dim} degree={self.degree}"

    def forward(self, inputs, size=1):
        # inputs [..., 3] in [-size, size] -> [..., degree^2]
        scaled = inputs / size
        lead = list(scaled.shape[:-1])
        flat = scaled.reshape(-1, self.input_dim)
        return sh_encode(flat, self.degree, flat.requires_grad).reshape(lead + [self.output_dim])
