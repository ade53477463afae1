"""Multiresolution hash-grid encoder: autograd Function + nn.Module with the reference's public
surface (gridencoder/grid.py:24-185): `grid_encode(...)`, `GridEncoder(input_dim, num_levels, level_dim,
per_level_scale, base_resolution, log2_hashmap_size, desired_resolution, gridtype, align_corners,
interpolation)`, `.forward(inputs, bound)`, `.grad_total_variation(...)`, parameter `embeddings`
[n_entries, level_dim] and buffer `offsets` [num_levels+1] (checkpoint-compatible names and shapes).

Differences that stay inside the op boundary:
  * the autocast decision, dtype flow and output layout ([B, L*C], level-major features) are the
    reference's; the kernels accumulate in fp32 and round once;
  * `torch.amp.custom_fwd/custom_bwd(device_type='cuda')` replace the deprecated torch.cuda.amp aliases.
"""
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

import _ngp_capi as _capi

try:  # the compiled binding first, as the reference does (gridencoder/grid.py:9-12); the ctypes binding of the same C ABI otherwise
    import os as _os
    if _os.environ.get('NGP_HIP_LIBRARY'):  # a variant library is selected: the compiled module links the in-tree one, the ctypes binding follows the variable
        raise ImportError('NGP_HIP_LIBRARY is set')
    import _gridencoder as _backend
except ImportError:
    from .backend import _backend

GRIDTYPE_IDS = {'hash': 0, 'tiled': 1}
INTERP_IDS = {'linear': 0, 'smoothstep': 1}


def level_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners):
    """Cumulative entry offsets of the levels (reference grid.py:112-129): level l has
    min(2^log2_hashmap_size, (ceil(H * s^l) + 1)^D) entries (no +1 with align_corners), rounded up to 8."""
    cap = 2 ** log2_hashmap_size
    sizes = []
    for lvl in range(num_levels):
        side = int(np.ceil(base_resolution * per_level_scale ** lvl)) + (0 if align_corners else 1)
        sizes.append(int(math.ceil(min(cap, side ** input_dim) / 8) * 8))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _wants_determinism(deterministic):
    """the module's `deterministic` when a backward runs: None follows PyTorch's determinism switch as it stands then.  False (the default of
    grid_encode) asks nothing of the host: the call runs what it always ran"""
    return torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)


def _ordered_backend():
    """gridencoder/backend.py, which holds scatter_path and the ordered entries' wrappers: loaded when a backward first asks for determinism,
    so that a process on the compiled `_gridencoder` module imports what it always imported"""
    from . import backend
    return backend


def _scatter_path(geometry, embeddings, offsets, deterministic, order):
    """scatter_path (gridencoder/backend.py) of a backward of this op"""
    n_points, dim, feat, n_levels, log2_scale, base_resolution, gridtype, interpolation, align_corners = geometry
    return _ordered_backend().scatter_path(n_points, dim, feat, n_levels, log2_scale, base_resolution, gridtype, align_corners, embeddings.dtype, deterministic,
                        order, offsets if order == 1 else None)


def _first_order_backward(grad, inputs, embeddings, offsets, dy_dx, geometry, deterministic=False):
    """d loss / d inputs (None without dy_dx) and d loss / d embeddings from the upstream gradient [B, L*C]; deterministic: the table
    gradient without float atomics where the call's own plan has them (scatter_path 'ordered': the same arguments, the ordered entry)"""
    n_points, dim, feat, n_levels, log2_scale, base_resolution, gridtype, interpolation, align_corners = geometry
    grad_level_major = grad.view(n_points, n_levels, feat).permute(1, 0, 2).contiguous()
    grad_embeddings = torch.zeros_like(embeddings)
    grad_inputs = torch.zeros_like(inputs, dtype=embeddings.dtype) if dy_dx is not None else None

    ordered = _wants_determinism(deterministic) and _scatter_path(geometry, embeddings, offsets, True, 1) == 'ordered'
    (_ordered_backend().grid_encode_backward_ordered if ordered else _backend.grid_encode_backward)(
        grad_level_major, inputs, embeddings, offsets, grad_embeddings, n_points, dim, feat, n_levels, log2_scale, base_resolution, dy_dx,
        grad_inputs, gridtype, align_corners, interpolation)
    if grad_inputs is not None:
        grad_inputs = grad_inputs.to(inputs.dtype)
    return grad_inputs, grad_embeddings


class _grid_encode(Function):
    @staticmethod
    @custom_fwd(device_type='cuda')
    def forward(ctx, inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs=False, gridtype=0,
                align_corners=False, interpolation=0, deterministic=False):
        # inputs [B, D] fp32 in [0, 1]; embeddings [n_entries, C]; offsets [L+1] int32 -> [B, L*C]
        inputs_src, table_src = inputs, embeddings
        inputs = inputs.contiguous()
        n_points, dim = inputs.shape
        n_levels = offsets.shape[0] - 1
        feat = embeddings.shape[1]
        log2_scale = np.log2(per_level_scale)

        # half-precision tables under autocast, but only for an even feature count (grid.py:41-44)
        if torch.is_autocast_enabled('cuda') and feat % 2 == 0:
            embeddings = embeddings.to(torch.half)
        embeddings = embeddings.contiguous()

        level_major = torch.empty(n_levels, n_points, feat, device=inputs.device, dtype=embeddings.dtype)
        dy_dx = torch.empty(n_points, n_levels * dim * feat, device=inputs.device, dtype=embeddings.dtype) if calc_grad_inputs else None

        _backend.grid_encode_forward(inputs, embeddings, offsets, level_major, n_points, dim, feat, n_levels, log2_scale,
                                     base_resolution, dy_dx, gridtype, align_corners, interpolation)

        ctx.save_for_backward(inputs, embeddings, offsets, dy_dx)
        # a copy made here (the half table of autocast, a contiguous copy of the inputs) is not part of the graph: a differentiable first
        # backward (create_graph=True) routes its gradients to the tensors the caller passed.  Plain references, not saved tensors: the
        # first-order backward neither reads them nor checks their version
        ctx.sources = (None if inputs_src is inputs else inputs_src, None if table_src is embeddings else table_src)
        ctx.geometry = (n_points, dim, feat, n_levels, log2_scale, base_resolution, gridtype, interpolation, align_corners)
        ctx.deterministic = deterministic
        return level_major.permute(1, 0, 2).reshape(n_points, n_levels * feat)

    @staticmethod
    @custom_bwd(device_type='cuda')
    def backward(ctx, grad):
        inputs, embeddings, offsets, dy_dx = ctx.saved_tensors
        if torch.is_grad_enabled():
            # create_graph=True (eikonal / SDF losses on d enc / d x): the same backend calls as a differentiable op
            grad_inputs, grad_embeddings = _grid_encode_backward.apply(grad, inputs, embeddings, offsets, dy_dx, ctx.geometry, *ctx.sources,
                                                                       ctx.deterministic)
        else:
            grad_inputs, grad_embeddings = _first_order_backward(grad, inputs, embeddings, offsets, dy_dx, ctx.geometry, ctx.deterministic)
        return grad_inputs, grad_embeddings, None, None, None, None, None, None, None, None


class _grid_encode_backward(Function):
    """The first backward of the grid encoder as an op of its own, so that its outputs (grad_inputs, grad_embeddings) can be differentiated:
    forward is _first_order_backward, as _grid_encode.backward (the same bits), backward is the second order (_grid_encode_second, DESIGN.md
    3.6)."""

    @staticmethod
    def forward(ctx, grad, inputs, embeddings, offsets, dy_dx, geometry, inputs_src=None, table_src=None, deterministic=False):
        # inputs_src / table_src: the tensors the encoder was called with when `inputs` / `embeddings` are copies of them (the half table of
        # autocast): the second-order gradients go there
        grad_inputs, grad_embeddings = _first_order_backward(grad, inputs, embeddings, offsets, dy_dx, geometry, deterministic)
        ctx.save_for_backward(grad, inputs, embeddings, offsets)
        ctx.geometry = geometry
        ctx.deterministic = deterministic
        ctx.sources = (inputs_src, table_src)
        # an output nobody differentiates (grad_embeddings in an eikonal loss, grad_inputs in a gradgradcheck over the table) reaches
        # backward as None, and its terms are skipped
        ctx.set_materialize_grads(False)
        return grad_inputs, grad_embeddings

    @staticmethod
    def backward(ctx, grad_grad_inputs, grad_grad_embeddings):
        grad, inputs, embeddings, offsets = ctx.saved_tensors
        inputs_src, table_src = ctx.sources
        need = ctx.needs_input_grad
        needs = (need[0], need[1] or need[6], need[2] or need[7])
        d_grad, d_inputs, d_embeddings = _grid_encode_second.apply(
            grad_grad_inputs, grad_grad_embeddings, grad, inputs if inputs_src is None else inputs_src,
            embeddings if table_src is None else table_src, inputs, embeddings, offsets, ctx.geometry, needs, ctx.deterministic)
        inputs_copied, table_copied = inputs_src is not None, table_src is not None
        return (d_grad, None if inputs_copied else d_inputs, None if table_copied else d_embeddings, None, None, None,
                d_inputs if inputs_copied else None, d_embeddings if table_copied else None, None)


class _grid_encode_second(Function):
    """Second order of the grid encoder.  With u = d loss / d grad_inputs and v = d loss / d grad_embeddings (either may be None):
      u-terms: ngp_grid_encode_backward_backward (one HIP pass: d/d table, d/d grad, d/d inputs);
      v-terms: the encoder forward on the table v (d/d grad) and the first backward's input term on the table v (d/d inputs).
    Its inputs include the upstream gradient, the points and the table the caller differentiates (inputs_anchor / table_anchor), so that
    differentiating its results once more reaches backward, which refuses third order."""

    @staticmethod
    def forward(ctx, grad_grad_inputs, grad_grad_embeddings, grad, inputs_anchor, table_anchor, inputs, embeddings, offsets, geometry, needs,
                deterministic=False):
        n_points, dim, feat, n_levels, log2_scale, base_resolution, gridtype, interpolation, align_corners = geometry
        need_grad, need_inputs, need_embeddings = needs
        dtype = embeddings.dtype
        d_grad = d_inputs = d_embeddings = None
        grad_level_major = grad.view(n_points, n_levels, feat).permute(1, 0, 2).contiguous()

        if grad_grad_inputs is not None and (need_grad or need_inputs or need_embeddings):
            # u-terms: one pass of the new kernels
            u = grad_grad_inputs.to(dtype).contiguous()
            d_embeddings = torch.zeros_like(embeddings)
            d_grad = torch.empty(n_levels, n_points, feat, device=inputs.device, dtype=dtype) if need_grad else None
            d_inputs = torch.empty(n_points, dim, device=inputs.device, dtype=dtype) if need_inputs else None
            ordered = _wants_determinism(deterministic) and _scatter_path(geometry, embeddings, offsets, True, 2) == 'ordered'
            (_ordered_backend().grid_encode_backward_backward_ordered if ordered else grid_encode_backward_backward)(
                grad_level_major, inputs, embeddings, offsets, u, d_grad, d_embeddings, d_inputs, n_points, dim, feat, n_levels, log2_scale,
                base_resolution, gridtype, align_corners, interpolation)
            if not need_embeddings:
                d_embeddings = None

        if grad_grad_embeddings is not None and (need_grad or need_inputs):
            # v-terms: the encoder on the table v (and its dy_dx), then the first backward's input term on that table
            v = grad_grad_embeddings.to(dtype).contiguous()
            enc_v = torch.empty(n_levels, n_points, feat, device=inputs.device, dtype=dtype)
            dy_dx_v = torch.empty(n_points, n_levels * dim * feat, device=inputs.device, dtype=dtype) if need_inputs else None
            _backend.grid_encode_forward(inputs, v, offsets, enc_v, n_points, dim, feat, n_levels, log2_scale, base_resolution, dy_dx_v,
                                         gridtype, align_corners, interpolation)
            if need_grad:
                d_grad = enc_v if d_grad is None else d_grad + enc_v
            if need_inputs:
                gx_v = torch.zeros(n_points, dim, device=inputs.device, dtype=dtype)
                unused = torch.zeros_like(v)   # (the entry also scatters w * grad into a table: not needed here)
                _backend.grid_encode_backward(grad_level_major, inputs, v, offsets, unused, n_points, dim, feat, n_levels, log2_scale,
                                              base_resolution, dy_dx_v, gx_v, gridtype, align_corners, interpolation)
                d_inputs = gx_v if d_inputs is None else d_inputs + gx_v

        if d_grad is not None:
            d_grad = d_grad.permute(1, 0, 2).reshape(n_points, n_levels * feat).to(grad.dtype)
        if d_inputs is not None:
            d_inputs = d_inputs.to(inputs.dtype)
        return d_grad, d_inputs, d_embeddings

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("grid_encode: third-order gradients are not provided (the grid encoder's second-order backward is not "
                           "differentiable)")


def grid_encode_backward_backward(grad, inputs, embeddings, offsets, u, grad_grad, grad_embeddings, grad_inputs2, B, D, C, L, S, H, gridtype,
                                  align_corners, interp):
    """ngp_grid_encode_backward_backward (include/ngp_hip.h) on tensors: grad [L,B,C], u [B,D] in the table dtype; grad_grad [L,B,C] and
    grad_inputs2 [B,D] written (None: not computed), grad_embeddings accumulated"""
    for t, name in ((grad, 'grad'), (inputs, 'inputs'), (embeddings, 'embeddings'), (offsets, 'offsets'), (u, 'grad_grad_inputs'),
                    (grad_embeddings, 'grad_embeddings'), (grad_grad, 'grad_grad'), (grad_inputs2, 'grad_inputs2')):
        if t is not None:
            _capi.dense(t, name)
    _capi.require_int32(offsets, 'offsets')
    if inputs.dtype != torch.float32:
        raise RuntimeError("expected scalar type Float for inputs but found " + str(inputs.dtype))
    for t, name in ((grad, 'grad'), (u, 'grad_grad_inputs'), (grad_embeddings, 'grad_embeddings'), (grad_grad, 'grad_grad'),
                    (grad_inputs2, 'grad_inputs2')):
        if t is not None and t.dtype != embeddings.dtype:
            raise RuntimeError(f"{name} must have the table's dtype {embeddings.dtype} (got {t.dtype})")
    code = _capi.float_code(embeddings, 'embeddings')
    nbytes = int(_capi.lib.ngp_grid_backward_backward_workspace_bytes(None, B, D, C, L, code))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=inputs.device) if nbytes else None
    _capi.check(_capi.lib.ngp_grid_encode_backward_backward(
        _capi.ptr(grad), _capi.ptr(inputs), _capi.ptr(embeddings), _capi.ptr(offsets), _capi.ptr(u), _capi.ptr(grad_grad),
        _capi.ptr(grad_embeddings), _capi.ptr(grad_inputs2), B, D, C, L, float(S), H, gridtype, int(bool(align_corners)), interp, code,
        _capi.ptr(ws), nbytes, _capi.stream()))


grid_encode = _grid_encode.apply


class GridEncoder(nn.Module):
    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19,
                 desired_resolution=None, gridtype='hash', align_corners=False, interpolation='linear', deterministic=None):
        # deterministic: the table gradient (first and second order) without float atomics, bit-reproducible.  None follows
        # torch.are_deterministic_algorithms_enabled() when the backward runs, True / False force the choice
        super().__init__()
        if desired_resolution is not None:
            # geometric progression from base_resolution to desired_resolution over the levels (grid.py:101-102)
            per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1))

        self.input_dim = input_dim
        self.num_levels = num_levels
        self.level_dim = level_dim
        self.per_level_scale = per_level_scale
        self.log2_hashmap_size = log2_hashmap_size
        self.base_resolution = base_resolution
        self.output_dim = num_levels * level_dim
        self.gridtype = gridtype
        self.gridtype_id = GRIDTYPE_IDS[gridtype]
        self.interpolation = interpolation
        self.interp_id = INTERP_IDS[interpolation]
        self.align_corners = align_corners
        self.deterministic = deterministic
        self.max_params = 2 ** log2_hashmap_size

        offsets = level_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size, align_corners)
        self.register_buffer('offsets', torch.from_numpy(offsets))
        self.n_params = int(offsets[-1]) * level_dim
        self.embeddings = nn.Parameter(torch.empty(int(offsets[-1]), level_dim))
        self.reset_parameters()

    def reset_parameters(self):
        self.embeddings.data.uniform_(-1e-4, 1e-4)  # grid.py:138-140

    def __repr__(self):
        finest = int(round(self.base_resolution * self.per_level_scale ** (self.num_levels - 1)))
        return (f"GridEncoder: input_dim={self.input_dim} num_levels={self.num_levels} level_dim={self.level_dim} "
                f"resolution={self.base_resolution} -> {finest} per_level_scale={self.per_level_scale:.4f} "
                f"params={tuple(self.embeddings.shape)} gridtype={self.gridtype} align_corners={self.align_corners} "
                f"interpolation={self.interpolation}")

    def forward(self, inputs, bound=1):
        # inputs [..., input_dim] in [-bound, bound] -> [..., num_levels * level_dim]
        fn = getattr(self.embeddings, '_ngp_materialize', None)
        if fn is not None:
            fn()   # optim.NGPAdam keeps this table in two buffer sets (enable_table_fusion): the Parameter becomes the current one (a no-op
                   # unless fused-table steps ran since the last call)
        unit = (inputs + bound) / (2 * bound)
        lead = list(unit.shape[:-1])
        flat = unit.view(-1, self.input_dim)
        out = grid_encode(flat, self.embeddings, self.offsets, self.per_level_scale, self.base_resolution, flat.requires_grad,
                          self.gridtype_id, self.align_corners, self.interp_id, self.deterministic)
        return out.view(lead + [self.output_dim])

    @torch.amp.autocast('cuda', enabled=False)
    def grad_total_variation(self, weight=1e-7, inputs=None, bound=1, B=1000000):
        """adds the total-variation gradient at `inputs` (or B random points) to embeddings.grad (grid.py:165-185)"""
        if self.embeddings.grad is None:
            raise ValueError('grad is None, should be called after loss.backward() and before optimizer.step()!')
        if inputs is None:
            pts = torch.rand(B, self.input_dim, device=self.embeddings.device, dtype=self.embeddings.dtype)   # (the op takes one dtype)
        else:
            pts = ((inputs + bound) / (2 * bound)).view(-1, self.input_dim)
            B = pts.shape[0]
        n_levels = self.offsets.shape[0] - 1
        _backend.grad_total_variation(pts.contiguous(), self.embeddings, self.embeddings.grad, self.offsets, weight, B,
                                      self.input_dim, self.embeddings.shape[1], n_levels, np.log2(self.per_level_scale),
                                      self.base_resolution, self.gridtype_id, self.align_corners)
