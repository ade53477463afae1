"""`_backend` of the grid encoder: the three callables the reference's pybind module exports
(gridencoder/src/bindings.cpp:5-9), same names, same positional arguments, tensors in place of
at::Tensor -- implemented by libngp_hip.so through its C ABI (include/ngp_hip.h).

A reference-style wrapper (`from .backend import _backend`, gridencoder/grid.py:9-12) works against this
object unchanged.
"""
import types

import _ngp_capi as capi


def _check_common(inputs, embeddings, offsets):
    capi.dense(inputs, 'inputs')
    capi.dense(embeddings, 'embeddings')
    capi.dense(offsets, 'offsets')
    capi.require_int32(offsets, 'offsets')
    if inputs.dtype != capi.torch.float32:
        # the reference reads inputs through data_ptr<float>() regardless of the dispatch type (gridencoder.cu:469)
        raise RuntimeError("expected scalar type Float for inputs but found " + str(inputs.dtype))


def grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx, gridtype, align_corners, interp):
    _check_common(inputs, embeddings, offsets)
    capi.dense(outputs, 'outputs')
    capi.float64_call((embeddings, 'embeddings'), (outputs, 'outputs'), (dy_dx, 'dy_dx'))
    code = capi.float_code(embeddings, 'embeddings')
    capi.check(capi.lib.ngp_grid_encode_forward(
        capi.ptr(inputs), capi.ptr(embeddings), capi.ptr(offsets), capi.ptr(outputs), B, D, C, L, float(S), H,
        capi.ptr(dy_dx), gridtype, int(bool(align_corners)), interp, code, capi.stream()))


def grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs,
                         gridtype, align_corners, interp):
    _check_common(inputs, embeddings, offsets)
    capi.dense(grad, 'grad')
    capi.dense(grad_embeddings, 'grad_embeddings')
    capi.float64_call((grad, 'grad'), (embeddings, 'embeddings'), (grad_embeddings, 'grad_embeddings'), (dy_dx, 'dy_dx'), (grad_inputs, 'grad_inputs'))
    code = capi.float_code(grad, 'grad')
    # large fp16 batches: the binned, atomic-free scatter needs scratch memory (include/ngp_hip.h, ngp_grid_encode_backward_ws); the
    # reference signature has no workspace argument, so it is allocated here
    arr, ws, nbytes = capi.grid_backward_workspace(offsets, B, D, C, L, S, H, gridtype, align_corners, code)
    capi.check(capi.lib.ngp_grid_encode_backward_ws(
        capi.ptr(grad), capi.ptr(inputs), capi.ptr(embeddings), capi.ptr(offsets), capi.ptr(grad_embeddings), B, D, C, L,
        float(S), H, capi.ptr(dy_dx), capi.ptr(grad_inputs), gridtype, int(bool(align_corners)), interp, code, 0.0,
        None if arr is None else capi.ctypes.cast(arr, capi.ctypes.c_void_p), capi.ptr(ws), nbytes, capi.stream()))


def _dtype_code(dtype):
    if isinstance(dtype, int):
        return dtype
    codes = {capi.torch.float32: capi.NGP_F32, capi.torch.float16: capi.NGP_F16, capi.torch.float64: capi.NGP_F64}
    if dtype not in codes:
        raise RuntimeError(f"scatter_path: the table dtype must be float32, float16 or float64 (got {dtype})")
    return codes[dtype]


def scatter_path(B, D, C, L, S, H, gridtype, align_corners, dtype, deterministic, order, offsets=None):
    """How the table gradient of a backward is scattered (host computation only): 'fp64' (the record sort of the fp64 path), 'sorted' (the
    first order's record-sort plan covers every level: already free of float atomics), 'ordered' (the ordered scatter) or
    'atomic'.  order: 1 = the first backward, 2 = the second-order one.  dtype: the table's (a torch dtype or an NGP_F* code).
    deterministic: True / False, None = torch.are_deterministic_algorithms_enabled() now.  offsets: the table's offsets (tensor, sequence or
    ctypes int32 array) -- the first order's plan depends on the level sizes; without them it counts as not reproducible, as a backward
    call without the host offsets runs."""
    if order not in (1, 2):
        raise ValueError(f"scatter_path: order must be 1 or 2 (got {order})")
    code = _dtype_code(dtype)
    if code == capi.NGP_F64:
        return 'fp64'
    if deterministic is None:
        deterministic = capi.torch.are_deterministic_algorithms_enabled()
    if order == 1 and offsets is not None:
        if isinstance(offsets, capi.torch.Tensor):
            arr = capi.host_offsets(offsets)
        elif isinstance(offsets, capi.ctypes.Array):
            arr = offsets
        else:
            arr = (capi.ctypes.c_int32 * len(offsets))(*[int(v) for v in offsets])
        if arr is not None and capi.lib.ngp_grid_backward_is_reproducible(capi.ctypes.cast(arr, capi.ctypes.c_void_p), B, D, C, L, float(S), H, gridtype,
                                                                          int(bool(align_corners)), code) == 1:
            return 'sorted'
    return 'ordered' if deterministic else 'atomic'


def _ordered_workspace(B, D, C, code, device):
    nbytes = int(capi.lib.ngp_grid_ordered_workspace_bytes(B, D, C, code))
    return (capi.torch.empty(nbytes, dtype=capi.torch.uint8, device=device) if nbytes else None), nbytes


def grid_encode_backward_ordered(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype,
                                 align_corners, interp):
    """grid_encode_backward with the ordered scatter (ngp_grid_encode_backward_ordered): the same arguments, bit-reproducible
    grad_embeddings, fp32 and fp16 tables"""
    _check_common(inputs, embeddings, offsets)
    capi.dense(grad, 'grad')
    capi.dense(grad_embeddings, 'grad_embeddings')
    code = capi.float_code(grad, 'grad')
    for t, name in ((grad_embeddings, 'grad_embeddings'), (dy_dx, 'dy_dx'), (grad_inputs, 'grad_inputs')):
        if t is not None and t.dtype != grad.dtype:
            raise RuntimeError(f"{name} must have the dtype of grad, {grad.dtype} (got {t.dtype})")
    ws, nbytes = _ordered_workspace(B, D, C, code, inputs.device)
    capi.check(capi.lib.ngp_grid_encode_backward_ordered(
        capi.ptr(grad), capi.ptr(inputs), capi.ptr(embeddings), capi.ptr(offsets), capi.ptr(grad_embeddings), B, D, C, L, float(S), H,
        capi.ptr(dy_dx), capi.ptr(grad_inputs), gridtype, int(bool(align_corners)), interp, code, 0.0, capi.ptr(ws), nbytes, capi.stream()))


def grid_encode_backward_backward_ordered(grad, inputs, embeddings, offsets, u, grad_grad, grad_embeddings, grad_inputs2, B, D, C, L, S, H,
                                          gridtype, align_corners, interp):
    """ngp_grid_encode_backward_backward_ordered on tensors, the arguments of grid.grid_encode_backward_backward"""
    _check_common(inputs, embeddings, offsets)
    for t, name in ((grad, 'grad'), (u, 'grad_grad_inputs'), (grad_embeddings, 'grad_embeddings'), (grad_grad, 'grad_grad'),
                    (grad_inputs2, 'grad_inputs2')):
        if t is not None:
            capi.dense(t, name)
            if t.dtype != embeddings.dtype:
                raise RuntimeError(f"{name} must have the table's dtype {embeddings.dtype} (got {t.dtype})")
    code = capi.float_code(embeddings, 'embeddings')
    ws, nbytes = _ordered_workspace(B, D, C, code, inputs.device)
    capi.check(capi.lib.ngp_grid_encode_backward_backward_ordered(
        capi.ptr(grad), capi.ptr(inputs), capi.ptr(embeddings), capi.ptr(offsets), capi.ptr(u), capi.ptr(grad_grad), capi.ptr(grad_embeddings),
        capi.ptr(grad_inputs2), B, D, C, L, float(S), H, gridtype, int(bool(align_corners)), interp, code, capi.ptr(ws), nbytes, capi.stream()))


def grad_total_variation(inputs, embeddings, grad, offsets, weight, B, D, C, L, S, H, gridtype, align_corners):
    capi.dense(inputs, 'inputs')
    capi.dense(embeddings, 'embeddings')
    capi.dense(grad, 'grad')
    capi.dense(offsets, 'offsets')
    capi.float64_call((inputs, 'inputs'), (embeddings, 'embeddings'), (grad, 'grad'))
    code = capi.float_code(embeddings, 'embeddings')
    if inputs.dtype != embeddings.dtype or grad.dtype != embeddings.dtype:
        raise RuntimeError("grad_total_variation: inputs, embeddings and grad must share one dtype")
    capi.check(capi.lib.ngp_grad_total_variation(
        capi.ptr(inputs), capi.ptr(embeddings), capi.ptr(grad), capi.ptr(offsets), float(weight), B, D, C, L, float(S), H,
        gridtype, int(bool(align_corners)), code, capi.stream()))


def grid_corner_indices(inputs, offsets, indices, B, D, L, S, H, gridtype, align_corners):
    """diagnostic extension, see include/ngp_hip.h"""
    capi.check(capi.lib.ngp_grid_corner_indices(capi.ptr(inputs), capi.ptr(offsets), capi.ptr(indices), B, D, L, float(S), H,
                                                gridtype, int(bool(align_corners)), capi.stream()))


_backend = types.SimpleNamespace(grid_encode_forward=grid_encode_forward, grid_encode_backward=grid_encode_backward,
                                 grad_total_variation=grad_total_variation, grid_corner_indices=grid_corner_indices)

__all__ = ['_backend']
