"""Frequency (positional) encoding  x -> [x, sin(2^0 x), cos(2^0 x), ..., sin(2^(deg-1) x), cos(2^(deg-1) x)]  on libngp_hip.so.

Public surface of the reference package (freqencoder/freq.py:15-77): `freq_encode(inputs, degree, output_dim)` and
`FreqEncoder(input_dim=3, degree=4)` with attributes `input_dim`, `degree`, `output_dim = input_dim * (1 + 2 * degree)` and a
`forward(inputs, **kwargs)` that accepts any leading shape.  Within each frequency the D sines come first, then the D cosines.
The op computes in fp32 (autocast inputs are widened) or, for float64 inputs, in fp64; its backward needs only the stored outputs,
because d sin(kx)/dx = k cos(kx) and d cos(kx)/dx = -k sin(kx) are already in there.  The first backward is differentiable
(torch.autograd.grad(..., create_graph=True), eikonal / normal losses): DESIGN.md 3.8.
"""
import torch
from torch import nn
from torch.amp import custom_bwd, custom_fwd

import _ngp_capi as _capi

try:  # the compiled binding first, as the reference does (freqencoder/freq.py:9-12); the ctypes binding of the same C ABI otherwise
    import os as _os
    if _os.environ.get('NGP_HIP_LIBRARY'):  # a variant library is selected: the compiled module links the in-tree one, the ctypes binding follows the variable
        raise ImportError('NGP_HIP_LIBRARY is set')
    import _freqencoder as _backend
except ImportError:
    from .backend import _backend


def encoded_width(input_dim, degree):
    return input_dim * (1 + 2 * degree)


def _forward_call(points, count, dim, degree, width, encoded):
    if points.dtype == torch.float64:   # the fp64 twins are reached through the C ABI; fp32 keeps the compiled binding
        _capi.check(_capi.lib.ngp_freq_encode_forward_f64(_capi.ptr(_capi.dense(points, 'inputs')), count, dim, degree, width,
                                                          _capi.ptr(_capi.dense(encoded, 'outputs')), _capi.stream()))
    else:
        _backend.freq_encode_forward(points, count, dim, degree, width, encoded)


def _first_order_backward(grad_encoded, encoded, geometry):
    count, dim, degree, width = geometry
    grad_points = encoded.new_empty((count, dim))  # the kernel overwrites every element
    grad_encoded = grad_encoded.contiguous()
    if encoded.dtype == torch.float64:
        _capi.float64_call((grad_encoded, 'grad'), (encoded, 'outputs'))
        _capi.check(_capi.lib.ngp_freq_encode_backward_f64(_capi.ptr(_capi.dense(grad_encoded, 'grad')), _capi.ptr(encoded), count, dim, degree,
                                                           width, _capi.ptr(grad_points), _capi.stream()))
    else:
        _backend.freq_encode_backward(grad_encoded, encoded, count, dim, degree, width, grad_points)
    return grad_points


def freq_encode_backward_backward(grad, outputs, u, B, D, deg, C, grad_grad, grad_inputs2):
    """ngp_freq_encode_backward_backward (include/ngp_hip.h) on tensors: grad [B,C], outputs [B,C], u [B,D]; grad_grad [B,C] and
    grad_inputs2 [B,D] overwritten (None: not computed).  All float32 or all float64."""
    for t, name in ((grad, 'grad'), (outputs, 'outputs'), (u, 'grad_grad_inputs'), (grad_grad, 'grad_grad'), (grad_inputs2, 'grad_inputs2')):
        if t is not None:
            _capi.dense(t, name)
            if t.dtype != outputs.dtype:
                raise RuntimeError(f"{name} must have the outputs' dtype {outputs.dtype} (got {t.dtype})")
    _capi.check(_capi.lib.ngp_freq_encode_backward_backward(_capi.ptr(grad), _capi.ptr(outputs), _capi.ptr(u), B, D, deg, C, _capi.ptr(grad_grad),
                                                            _capi.ptr(grad_inputs2), _capi.float_code(outputs, 'outputs'), _capi.stream()))


class FrequencyEncoding(torch.autograd.Function):
    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, points, degree, width, caller=None):
        # the tensor of the graph: the caller's own (under autocast `points` is custom_fwd's fp32 copy of it).  A plain reference, not a
        # saved tensor: the first-order backward neither reads it nor checks its version
        ctx.source = points if caller is None else caller.tensor
        points = (points if points.is_cuda else points.cuda()).contiguous()
        count, dim = points.shape
        encoded = points.new_empty((count, width))
        _forward_call(points, count, dim, degree, width, encoded)
        ctx.save_for_backward(encoded)
        ctx.geometry = (count, dim, degree, width)
        return encoded

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, grad_encoded):
        (encoded,) = ctx.saved_tensors
        if torch.is_grad_enabled():
            # create_graph=True (eikonal / SDF losses on d enc / d x): the same backend call as a differentiable op
            grad_points = _freq_backward.apply(grad_encoded, encoded.detach(), ctx.geometry, ctx.source)
        else:
            grad_points = _first_order_backward(grad_encoded, encoded, ctx.geometry)
        return grad_points, None, None, None


class _freq_backward(torch.autograd.Function):
    """The first backward of the frequency encoder as an op of its own, so that its result can be differentiated: forward is
    _first_order_backward, as FrequencyEncoding.backward (the same bits), backward is the second order (_freq_second).
    `source` is the tensor the encoder was called with: the stored outputs are a function of it, and d/d source is returned for it."""

    @staticmethod
    def forward(ctx, grad_encoded, encoded, geometry, source):
        grad_points = _first_order_backward(grad_encoded, encoded, geometry)
        ctx.save_for_backward(grad_encoded, encoded)
        ctx.geometry = geometry
        ctx.source = source
        ctx.set_materialize_grads(False)   # a result nobody differentiates reaches backward as None: nothing is launched
        return grad_points

    @staticmethod
    def backward(ctx, u):
        if u is None:
            return None, None, None, None
        grad_encoded, encoded = ctx.saved_tensors
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[3])
        d_grad, d_source = _freq_second.apply(u, grad_encoded, encoded, ctx.source, ctx.geometry, needs)
        return d_grad, None, None, d_source


class _freq_second(torch.autograd.Function):
    """Second order of the frequency encoder: one call of ngp_freq_encode_backward_backward.  Its inputs include the upstream gradient
    and the points the caller differentiates, so that differentiating its results once more reaches backward, which refuses third order."""

    @staticmethod
    def forward(ctx, u, grad_encoded, encoded, source, geometry, needs):
        count, dim, degree, width = geometry
        need_grad, need_source = needs
        d_grad = encoded.new_empty((count, width)) if need_grad else None
        d_source = encoded.new_empty((count, dim)) if need_source else None
        if need_grad or need_source:
            freq_encode_backward_backward(grad_encoded.to(encoded.dtype).contiguous(), encoded, u.to(encoded.dtype).contiguous(), count, dim, degree,
                                          width, d_grad, d_source)
        if d_grad is not None:
            d_grad = d_grad.to(grad_encoded.dtype)
        if d_source is not None:
            d_source = d_source.to(device=source.device, dtype=source.dtype)   # an autocast caller's fp16 points get an fp16 gradient
        return d_grad, d_source

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("freq_encode: third-order gradients are not provided (the frequency encoder's second-order backward is not "
                           "differentiable)")


def freq_encode(inputs, degree, output_dim):
    return FrequencyEncoding.apply(inputs, degree, output_dim, _capi.CallerTensor(inputs))


class FreqEncoder(nn.Module):
    def __init__(self, input_dim=3, degree=4):
        super().__init__()
        self.input_dim, self.degree = input_dim, degree
        self.output_dim = encoded_width(input_dim, degree)

    def extra_repr(self):
        return f"input_dim={self.input_dim}, degree={self.degree}, output_dim={self.output_dim}"

    def forward(self, inputs, **kwargs):
        flat = inputs.reshape(-1, self.input_dim)
        return freq_encode(flat, self.degree, self.output_dim).reshape(*inputs.shape[:-1], self.output_dim)
