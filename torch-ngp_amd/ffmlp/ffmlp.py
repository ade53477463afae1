"""Fully fused fp16 MLP with the reference's surface (ffmlp/ffmlp.py:15-168):
`FFMLP(input_dim, output_dim, hidden_dim, num_layers, activation='relu')`, one flat fp32 parameter
`weights` laid out W_in [hid,in] | (num_layers-1) x W_h [hid,hid] | W_out [16,hid] (each [out,in] row
major), seed-42 uniform(+-sqrt(3/hidden)) init, batch padded to a multiple of 128 and outputs padded to
16 columns inside forward.  `num_layers` counts hidden layers (num_layers + 1 matmuls).

The backward_buffer the reference allocates as scratch is kept (same shape, zero-initialised) and
handed to the library, which uses it for its per-workgroup weight-gradient slabs.

Second order (no reference counterpart): under `torch.autograd.grad(y, x, create_graph=True)` the first backward runs as
an op of its own (`_ffmlp_backward`, the same backend call and the same bits) whose grad_inputs can be differentiated -- eikonal and
normal losses train the weights and whatever produced the inputs.  A loss on the weights' first-order gradient, and third order, raise.
"""
import math

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

import _ngp_capi as _capi

try:  # the compiled binding first, as the reference does (ffmlp/ffmlp.py:9-12); the ctypes binding of the same C ABI otherwise
    import os as _os
    if _os.environ.get('NGP_HIP_LIBRARY'):  # a variant library is selected: the compiled module links the in-tree one, the ctypes binding follows the variable
        raise ImportError('NGP_HIP_LIBRARY is set')
    import _ffmlp as _backend
except ImportError:
    from .backend import _backend

ACTIVATION_IDS = {'relu': 0, 'exponential': 1, 'sine': 2, 'sigmoid': 3, 'squareplus': 4, 'softplus': 5}


def convert_activation(act):
    """name -> id of ffmlp/src/utils.h:29-37; anything unknown (including 'none') is 6 = None"""
    return ACTIVATION_IDS.get(act, 6)


class _ffmlp_forward(Function):
    @staticmethod
    @custom_fwd(device_type='cuda', cast_inputs=torch.half)
    def forward(ctx, inputs, weights, input_dim, output_dim, hidden_dim, num_layers, activation, output_activation,
                inference=False, calc_grad_inputs=False, sources=None):
        # sources: the tensors the caller passed, before cast_inputs made half copies of them (ffmlp_forward below)
        inputs_src, weights_src = (inputs, weights) if sources is None else (sources.inputs, sources.weights)
        # a copy made on the way here (the half weights of autocast, a contiguous copy) is not part of the graph: a differentiable first
        # backward (create_graph=True) routes its gradients to the tensors the caller passed.  Plain references, not saved tensors, as in the
        # grid encoder: the first-order backward neither reads them nor checks their version
        inputs, weights = inputs.contiguous(), weights.contiguous()
        ctx.sources = (None if inputs_src is inputs else inputs_src, None if weights_src is weights else weights_src)
        batch = inputs.shape[0]
        outputs = torch.empty(batch, output_dim, device=inputs.device, dtype=inputs.dtype)
        if inference:
            scratch = torch.empty(batch, hidden_dim, device=inputs.device, dtype=inputs.dtype)
            _backend.ffmlp_inference(inputs, weights, batch, input_dim, output_dim, hidden_dim, num_layers, activation,
                                     output_activation, scratch, outputs)
            return outputs
        forward_buffer = torch.empty(num_layers, batch, hidden_dim, device=inputs.device, dtype=inputs.dtype)
        _backend.ffmlp_forward(inputs, weights, batch, input_dim, output_dim, hidden_dim, num_layers, activation,
                               output_activation, forward_buffer, outputs)
        ctx.save_for_backward(inputs, weights, forward_buffer)
        ctx.net = (input_dim, output_dim, hidden_dim, num_layers, activation, output_activation, calc_grad_inputs)
        return outputs

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, grad):
        inputs, weights, forward_buffer = ctx.saved_tensors
        grad = grad.contiguous()
        if torch.is_grad_enabled():
            # create_graph=True (eikonal / SDF losses on d y / d x): the same backend call as a differentiable op
            grad_inputs, grad_weights = _ffmlp_backward.apply(grad, inputs, weights, forward_buffer, ctx.net, *ctx.sources)
        else:
            grad_inputs, grad_weights = _first_order_backward(grad, inputs, weights, forward_buffer, ctx.net)
        return grad_inputs, grad_weights, None, None, None, None, None, None, None, None, None


def _first_order_backward(grad, inputs, weights, forward_buffer, net):
    """d loss / d inputs (None without calc_grad_inputs) and d loss / d weights from the upstream gradient [B, 16]"""
    input_dim, output_dim, hidden_dim, num_layers, activation, output_activation, calc_grad_inputs = net
    batch = grad.shape[0]
    # (the reference zero-fills these three, ffmlp.py:66-71; every kernel behind ffmlp_backward OVERWRITES what it is handed --
    # include/ngp_hip.h -- so the fills, one of them [num_layers, B, hidden], would be three launches per network for nothing)
    grad_inputs = torch.empty_like(inputs) if calc_grad_inputs else torch.empty(1, device=grad.device, dtype=grad.dtype)
    grad_weights = torch.empty_like(weights)
    backward_buffer = torch.empty(num_layers, batch, hidden_dim, device=grad.device, dtype=grad.dtype)
    _backend.ffmlp_backward(grad, inputs, weights, forward_buffer, batch, input_dim, output_dim, hidden_dim, num_layers,
                            activation, output_activation, calc_grad_inputs, backward_buffer, grad_inputs, grad_weights)
    return (grad_inputs if calc_grad_inputs else None), grad_weights


class _ffmlp_backward(Function):
    """The first backward of the MLP as an op of its own, so that grad_inputs can be differentiated: forward is _first_order_backward, as
    _ffmlp_forward.backward (the same bits), backward is the second order (_ffmlp_second)."""

    @staticmethod
    def forward(ctx, grad, inputs, weights, forward_buffer, net, inputs_src=None, weights_src=None):
        # inputs_src / weights_src: the tensors the network was called with when `inputs` / `weights` are copies of them (the half weights
        # of autocast): the second-order gradients go there
        grad_inputs, grad_weights = _first_order_backward(grad, inputs, weights, forward_buffer, net)
        ctx.save_for_backward(grad, inputs, weights, forward_buffer)
        ctx.net = net
        ctx.sources = (inputs_src, weights_src)
        # an output nobody differentiates (grad_weights in an eikonal loss) reaches backward as None
        ctx.set_materialize_grads(False)
        return grad_inputs, grad_weights

    @staticmethod
    def backward(ctx, grad_grad_inputs, grad_grad_weights):
        if grad_grad_weights is not None:
            raise RuntimeError("ffmlp: second order with respect to grad_weights is not provided (a loss on the weights' first-order "
                               "gradient); only grad_inputs can be differentiated")
        if grad_grad_inputs is None:
            return None, None, None, None, None, None, None
        grad, inputs, weights, forward_buffer = ctx.saved_tensors
        inputs_src, weights_src = ctx.sources
        need = ctx.needs_input_grad
        needs = (need[0], need[1] or need[5], need[2] or need[6])
        d_grad, d_inputs, d_weights = _ffmlp_second.apply(
            grad_grad_inputs, grad, inputs if inputs_src is None else inputs_src, weights if weights_src is None else weights_src,
            inputs, weights, forward_buffer, ctx.net, needs)
        inputs_copied, weights_copied = inputs_src is not None, weights_src is not None
        return (d_grad, None if inputs_copied else d_inputs, None if weights_copied else d_weights, None, None,
                d_inputs if inputs_copied else None, d_weights if weights_copied else None)


class _ffmlp_second(Function):
    """Second order of the MLP: with u = d loss / d grad_inputs, ngp_ffmlp_backward_backward gives d loss / d grad, d loss / d inputs and
    d loss / d weights.  Its inputs include the upstream gradient, the inputs and the weights the caller differentiates (inputs_anchor /
    weights_anchor), so that differentiating its results once more reaches backward, which refuses third order."""

    @staticmethod
    def forward(ctx, grad_grad_inputs, grad, inputs_anchor, weights_anchor, inputs, weights, forward_buffer, net, needs):
        input_dim, output_dim, hidden_dim, num_layers, activation, output_activation, calc_grad_inputs = net
        need_grad, need_inputs, need_weights = needs
        if not (need_grad or need_inputs or need_weights):
            return None, None, None
        u = grad_grad_inputs.to(torch.half).contiguous()
        d_grad = torch.empty_like(grad) if need_grad else None
        d_inputs = torch.empty_like(inputs) if need_inputs else None
        d_weights = torch.empty_like(weights) if need_weights else None
        ffmlp_backward_backward(grad, inputs, weights, forward_buffer, u, grad.shape[0], input_dim, output_dim, hidden_dim, num_layers,
                                activation, d_grad, d_weights, d_inputs)
        return d_grad, d_inputs, d_weights

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("ffmlp: third-order gradients are not provided (the MLP's second-order backward is not differentiable)")


def ffmlp_backward_backward(grad, inputs, weights, forward_buffer, u, B, input_dim, output_dim, hidden_dim, num_layers, activation,
                            grad_grad, grad_weights2, grad_inputs2):
    """ngp_ffmlp_backward_backward (include/ngp_hip.h) on fp16 tensors: grad [B,16], inputs and u [B,input_dim], forward_buffer as the
    forward left it; grad_grad [B,16], grad_weights2 [n_params] and grad_inputs2 [B,input_dim] are written (None: not computed)"""
    for t, name in ((grad, 'grad'), (inputs, 'inputs'), (weights, 'weights'), (forward_buffer, 'forward_buffer'), (u, 'grad_grad_inputs'),
                    (grad_grad, 'grad_grad'), (grad_weights2, 'grad_weights2'), (grad_inputs2, 'grad_inputs2')):
        if t is not None:
            _capi.dense(t, name)
            if t.dtype != torch.float16:
                raise RuntimeError(f"{name} must be a Half tensor")
    nbytes = int(_capi.lib.ngp_ffmlp_backward_backward_workspace_bytes(B, input_dim, hidden_dim, num_layers, activation))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=grad.device) if nbytes else None
    _capi.check(_capi.lib.ngp_ffmlp_backward_backward(_capi.ptr(grad), _capi.ptr(inputs), _capi.ptr(weights), _capi.ptr(forward_buffer),
                                                      _capi.ptr(u), B, input_dim, output_dim, hidden_dim, num_layers, activation,
                                                      _capi.ptr(grad_grad), _capi.ptr(grad_weights2), _capi.ptr(grad_inputs2), _capi.ptr(ws),
                                                      nbytes, _capi.stream()))


class _Sources:
    """the tensors a caller passed to ffmlp_forward, in a wrapper custom_fwd's cast_inputs leaves alone"""
    __slots__ = ('inputs', 'weights')

    def __init__(self, inputs, weights):
        self.inputs, self.weights = inputs, weights


def ffmlp_forward(inputs, weights, input_dim, output_dim, hidden_dim, num_layers, activation, output_activation, inference=False,
                  calc_grad_inputs=False):
    return _ffmlp_forward.apply(inputs, weights, input_dim, output_dim, hidden_dim, num_layers, activation, output_activation, inference,
                                calc_grad_inputs, _Sources(inputs, weights))


class FFMLP(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_dim, num_layers, activation='relu'):
        super().__init__()
        assert hidden_dim in [16, 32, 64, 128, 256], f"FFMLP only support hidden_dim in [16, 32, 64, 128, 256], but got {hidden_dim}"
        assert input_dim > 0 and input_dim % 16 == 0, f"FFMLP input_dim should be 16 * m (m  > 0), but got {input_dim}"
        assert output_dim <= 16, f"FFMLP current only supports output dim <= 16, but got {output_dim}"
        assert num_layers >= 2, f"FFMLP num_layers should be larger than 2 (3 matmuls), but got {num_layers}"

        self.input_dim = input_dim
        self.output_dim = output_dim
        self.hidden_dim = hidden_dim
        self.num_layers = num_layers
        self.activation = convert_activation(activation)
        self.output_activation = convert_activation('none')
        self.tensorcore_width = 16
        self.padded_output_dim = int(math.ceil(output_dim / 16)) * 16

        self.num_parameters = hidden_dim * (input_dim + hidden_dim * (num_layers - 1) + self.padded_output_dim)
        self.weights = nn.Parameter(torch.zeros(self.num_parameters))
        self.reset_parameters()
        _backend.allocate_splitk(self.num_layers + 1)  # kept for interface parity (ffmlp.py:126)

    def cleanup(self):
        _backend.free_splitk()

    def __repr__(self):
        return (f"FFMLP: input_dim={self.input_dim} output_dim={self.output_dim} hidden_dim={self.hidden_dim} "
                f"num_layers={self.num_layers} activation={self.activation}")

    def reset_parameters(self):
        torch.manual_seed(42)  # the reference reseeds the global generator here (ffmlp.py:141-144); kept for identical inits
        bound = math.sqrt(3 / self.hidden_dim)
        self.weights.data.uniform_(-bound, bound)

    def forward(self, inputs):
        # inputs [B, input_dim] -> [B, output_dim]
        batch, width = inputs.shape
        pad = 128 - (batch % 128)  # always pads, a whole 128 rows when already aligned (ffmlp.py:157-159)
        padded = torch.cat([inputs, torch.zeros(pad, width, dtype=inputs.dtype, device=inputs.device)], dim=0)
        out = ffmlp_forward(padded, self.weights, self.input_dim, self.padded_output_dim, self.hidden_dim, self.num_layers,
                            self.activation, self.output_activation, not self.training, padded.requires_grad)
        return out[:batch, :self.output_dim]
