"""CPU checks of the ordered scatter's entry points (include/ngp_hip.h: ngp_grid_encode_backward_ordered,
ngp_grid_encode_backward_backward_ordered, ngp_grid_ordered_workspace_bytes, ngp_grid_backward_is_reproducible): declared, exported and
bound; the ABI version unchanged; host-side validation (codes and messages, before any launch: no GPU needed); the workspace formula; the
reproducibility query and scatter_path; the built objects of the unit and of the record sort's (no scratch, no spills, no last-register 64-bit shift, no float
atomics and no compare-and-swap in any kernel)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import grid_backward_path_cases as gbp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['ngp_grid_encode_backward_ordered', 'ngp_grid_encode_backward_backward_ordered', 'ngp_grid_ordered_workspace_bytes',
           'ngp_grid_backward_is_reproducible']


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
    sig = capi._SIGNATURES
    # ..._backward_ws without offsets_host; ..._backward_backward as it is
    ws = sig['ngp_grid_encode_backward_ws']
    assert sig['ngp_grid_encode_backward_ordered'] == ws[:18] + ws[19:] and len(sig['ngp_grid_encode_backward_ordered']) == 21
    assert sig['ngp_grid_encode_backward_backward_ordered'] == sig['ngp_grid_encode_backward_backward']
    for name in ENTRIES[:2] + ENTRIES[3:]:
        assert getattr(capi.lib, name).argtypes == sig[name]
    assert capi.lib.ngp_grid_ordered_workspace_bytes.restype == ctypes.c_size_t
    for name in ENTRIES:
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read(), name


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def _a256(x):
    return (x + 255) & ~255


def _formula(B, D, C):
    n = B << D
    total = 4 * _a256(4 * n) + _a256(4 * (256 * 1024 + 256))
    m = n
    while m > 64:
        m = 2 * -(-m // 64)
        total += _a256(4 * m) + _a256(4 * C * m)
    return total


def test_workspace_formula():
    import _ngp_capi as capi
    ws = lambda B, D=3, C=2, dtype=capi.NGP_F32: int(capi.lib.ngp_grid_ordered_workspace_bytes(B, D, C, dtype))
    for B, D, C in ((1, 2, 1), (7, 2, 8), (16, 2, 2), (17, 2, 2), (1000, 5, 4), (4133, 3, 2), (1 << 18, 3, 2), (1 << 26, 5, 8)):
        assert ws(B, D, C) == ws(B, D, C, capi.NGP_F16) == _formula(B, D, C) > 0
        assert ws(B, D, C) % 256 == 0
    assert ws(0) == 0
    sizes = [ws(B) for B in (1, 2, 8, 9, 63, 64, 65, 512, 513, 4096, 4133, 1 << 18, (1 << 18) + 1)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                       # monotone in B
    # arguments the entries refuse: no workspace
    assert ws(64, D=6) == 0 and ws(64, D=1) == 0 and ws(64, C=3) == 0 and ws(64, dtype=capi.NGP_F64) == 0 and ws(64, dtype=7) == 0
    assert ws(1 << 28, D=3) == _formula(1 << 28, 3, 2) and ws((1 << 28) + 1, D=3) == 0   # B * 2^D <= 2^31
    # the existing query is untouched: fp16 / fp32 second order asks for no scratch
    assert int(capi.lib.ngp_grid_backward_backward_workspace_bytes(None, 1 << 18, 3, 2, 16, capi.NGP_F32)) == 0
    assert int(capi.lib.ngp_grid_backward_backward_workspace_bytes(None, 1 << 18, 3, 2, 16, capi.NGP_F16)) == 0


def _first(lib, B=8, D=3, C=2, L=2, dtype=0, ptrs=None, ws=ctypes.c_void_p(256), nbytes=1 << 40, bound=0.0):
    one = ctypes.c_void_p(256)
    p = [one, one, one, one, one, None, None] if ptrs is None else ptrs   # grad, inputs, embeddings, offsets, grad_embeddings, dy_dx, grad_inputs
    return lib.ngp_grid_encode_backward_ordered(p[0], p[1], p[2], p[3], p[4], B, D, C, L, 1.0, 4, p[5], p[6], 0, 0, 0, dtype, bound, ws, nbytes, None)


def _second(lib, B=8, D=3, C=2, L=2, dtype=0, ptrs=None, ws=ctypes.c_void_p(256), nbytes=1 << 40):
    one = ctypes.c_void_p(256)
    p = [one] * 8 if ptrs is None else ptrs
    return lib.ngp_grid_encode_backward_backward_ordered(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], B, D, C, L, 1.0, 4, 0, 0, 0, dtype, ws,
                                                         nbytes, None)


@pytest.mark.parametrize('which', ['first', 'second'])
def test_host_validation(which):
    import _ngp_capi as capi
    lib, F16, F32, F64 = capi.lib, capi.NGP_F16, capi.NGP_F32, capi.NGP_F64
    call = _first if which == 'first' else _second
    fn = b'grid_encode_backward_ordered' if which == 'first' else b'grid_encode_backward_backward_ordered'
    one = ctypes.c_void_p(256)
    err = lambda: lib.ngp_last_error()
    assert call(lib, D=6) == 1 and err().startswith(fn + b':') and b'input dim D must be 2, 3, 4 or 5 (got 6)' in err()
    assert call(lib, D=1) == 1 and b'input dim' in err()
    assert call(lib, C=3) == 1 and b'C must be 1, 2, 4, or 8. (got 3)' in err()
    assert call(lib, L=0) == 1 and b'number of levels must be in [1, 32] (got 0)' in err()
    assert call(lib, L=33) == 1 and b'number of levels' in err()
    assert call(lib, dtype=7) == 1 and b'embeddings must be float32 or float16' in err()
    # float64: refused, with the entry that serves it
    assert call(lib, dtype=F64) == 1 and b'float64 is not provided by this entry point' in err()
    assert (b'ngp_grid_encode_backward_ws' if which == 'first' else b'ngp_grid_encode_backward_backward') in err()
    # B == 0 is a no-op, whatever the pointers and the workspace
    n_ptrs = 7 if which == 'first' else 8
    assert call(lib, B=0, ptrs=[None] * n_ptrs, ws=None, nbytes=0) == 0
    # NULL tensors (embeddings is not read by the first order; the optional outputs may be NULL)
    needed = (0, 1, 3, 4) if which == 'first' else (0, 1, 2, 3, 4, 6)
    for i in needed:
        p = [one, one, one, one, one, None, None] if which == 'first' else [one] * 8
        p[i] = None
        assert call(lib, ptrs=p) == 1 and b'NULL tensor' in err(), i
    if which == 'first':
        # embeddings may be NULL: the call gets past the tensor check and stops at the next one, the workspace (still before any launch)
        assert call(lib, ptrs=[one, one, None, one, one, None, None], ws=None, nbytes=0) == 1 and b'needs a workspace' in err()
        assert call(lib, ptrs=[one, one, one, one, one, one, None]) == 1 and b'dy_dx and grad_inputs must both be given or both be NULL' in err()
        assert call(lib, ptrs=[one, one, one, one, one, one, one], bound=2.0) == 1 and b'fused input mapping does not provide grad_inputs' in err()
    # fp16 with odd C is accepted (nothing is packed): the next check, the workspace, is the one that fails
    assert call(lib, C=1, dtype=F16, ws=None, nbytes=0) == 1 and b'needs a workspace' in err()
    # the record limit, the workspace size and its alignment
    assert call(lib, B=(1 << 26) + 1, D=5) == 1 and b'B * 2^D must not exceed 2^31' in err()
    need = int(lib.ngp_grid_ordered_workspace_bytes(8, 3, 2, F32))
    assert call(lib, ws=None, nbytes=need) == 1 and b'needs a workspace of %d bytes (ngp_grid_ordered_workspace_bytes), got 0' % need in err()
    assert call(lib, nbytes=need - 1) == 1 and b'needs a workspace of %d bytes' % need in err() and b'got %d' % (need - 1) in err()
    assert call(lib, ws=ctypes.c_void_p(256 + 64), nbytes=need) == 1 and b'workspace must be 256-byte aligned' in err()


def _host(offs):
    arr = (ctypes.c_int32 * len(offs))(*[int(v) for v in offs])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


# (offsets of, B, D, C, dtype name) -> is the existing backward free of float atomics
def _query_cases():
    import _ngp_capi as capi
    t1, t2, t3 = gbp.table('T1'), gbp.table('T2'), gbp.table('T3')
    return [
        (t1, 16384, 3, 2, capi.NGP_F16, 1), (t2, 16384, 2, 2, capi.NGP_F16, 1), (t1, 16421, 3, 2, capi.NGP_F16, 1),
        (t3, 16384, 3, 2, capi.NGP_F16, 0),          # its level 1 is too large for the bins: atomics
        (t1, 16383, 3, 2, capi.NGP_F16, 0),          # below the record sort's smallest batch
        (t1, 16384, 3, 2, capi.NGP_F32, 0),          # fp32 tables
        (t1, 16384, 3, 4, capi.NGP_F16, 0),          # C != 2
        (t1, 4096, 4, 4, capi.NGP_F32, 0),           # fp32, C = 4, D = 4, B = 4096
        (t1, 4096, 4, 4, capi.NGP_F64, 1), (t3, 7, 3, 2, capi.NGP_F64, 1),   # fp64: always the record sort of the fp64 path
    ]


def test_reproducibility_query():
    import _ngp_capi as capi
    for tab, B, D, C, dtype, want in _query_cases():
        arr, hp = _host(tab['offs'])
        assert capi.lib.ngp_grid_backward_is_reproducible(hp, B, D, C, tab['L'], tab['S'], tab['H'], 0, 0, dtype) == want, (tab['name'], B, D, C, dtype)
    t1 = gbp.table('T1')
    arr, hp = _host(t1['offs'])
    q = lambda **kw: capi.lib.ngp_grid_backward_is_reproducible(*[kw.get(k, v) for k, v in dict(
        offs=hp, B=16384, D=3, C=2, L=t1['L'], S=t1['S'], H=t1['H'], gridtype=0, align=0, dtype=capi.NGP_F16).items()])
    assert q() == 1
    assert q(offs=None) == 0                                  # without the host offsets the backward cannot plan the sort
    assert q(L=0) == 0 and q(L=33) == 0 and q(D=6) == 0 and q(C=3) == 0
    assert q(offs=None, dtype=capi.NGP_F64) == 1


def test_scatter_path():
    import torch
    import _ngp_capi as capi
    from gridencoder import backend, grid
    dtypes = {capi.NGP_F16: torch.float16, capi.NGP_F32: torch.float32, capi.NGP_F64: torch.float64}
    for tab, B, D, C, code, reproducible in _query_cases():
        args = (B, D, C, tab['L'], tab['S'], tab['H'], 0, False, dtypes[code])
        for det in (False, True):
            first = backend.scatter_path(*args, det, 1, tab['offs'])
            second = backend.scatter_path(*args, det, 2, tab['offs'])
            if code == capi.NGP_F64:
                assert (first, second) == ('fp64', 'fp64')
                continue
            assert first == ('sorted' if reproducible else 'ordered' if det else 'atomic'), (tab['name'], B, D, C, code, det)
            assert second == ('ordered' if det else 'atomic')
            # without the offsets the first order's plan counts as not reproducible, as a backward without the host offsets runs
            assert backend.scatter_path(*args, det, 1) == ('ordered' if det else 'atomic')
        assert backend.scatter_path(*args[:8], code, False, 1, list(tab['offs'])) == backend.scatter_path(*args, False, 1, tab['offs'])
    # deterministic=None follows PyTorch's switch at the time of the call
    t1 = gbp.table('T1')
    args = (4096, 3, 2, t1['L'], t1['S'], t1['H'], 0, False, torch.float32)
    assert not torch.are_deterministic_algorithms_enabled()
    assert backend.scatter_path(*args, None, 1, t1['offs']) == 'atomic' and backend.scatter_path(*args, None, 2) == 'atomic'
    torch.use_deterministic_algorithms(True)
    try:
        assert backend.scatter_path(*args, None, 1, t1['offs']) == 'ordered' and backend.scatter_path(*args, None, 2) == 'ordered'
        assert backend.scatter_path(*args, False, 1, t1['offs']) == 'atomic'
        sorted_args = (16384, 3, 2, t1['L'], t1['S'], t1['H'], 0, False, torch.float16)
        assert backend.scatter_path(*sorted_args, None, 1, t1['offs']) == 'sorted'   # determinism it already has: the same path
    finally:
        torch.use_deterministic_algorithms(False)
    with pytest.raises(ValueError):
        backend.scatter_path(*args, True, 3)
    with pytest.raises(RuntimeError):
        backend.scatter_path(*args[:8], torch.int32, True, 1)


def test_module_keyword():
    import inspect
    from gridencoder import grid
    params = list(inspect.signature(grid.GridEncoder.__init__).parameters.values())
    assert params[-1].name == 'deterministic' and params[-1].default is None
    assert [p.name for p in params[1:-1]] == ['input_dim', 'num_levels', 'level_dim', 'per_level_scale', 'base_resolution', 'log2_hashmap_size',
                                              'desired_resolution', 'gridtype', 'align_corners', 'interpolation']
    fwd = list(inspect.signature(grid._grid_encode.forward).parameters.values())
    assert fwd[-1].name == 'deterministic' and fwd[-1].default is False
    enc = grid.GridEncoder(num_levels=2, log2_hashmap_size=8)
    assert enc.deterministic is None and grid.GridEncoder(num_levels=2, log2_hashmap_size=8, deterministic=True).deterministic is True


def _objects(unit):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    objs = [os.path.join(ROOT, 'torch-ngp_amd', 'csrc', d, unit + '.o') for d in ('_obj', '_obj_dbg')]
    if not isa.tools_present() or not all(os.path.exists(o) for o in objs):
        pytest.skip(unit + '.o (run __graft_entry__.build()) or the LLVM tools are missing')
    return isa, objs


# 64 sums of the records (2 dtypes x 16 (D, C) x 2 orders), 8 sums of partial sums (2 dtypes x 4 C), 32 gather-only instantiations of the
# second order's kernel, 2 input-gradient kernels; the record sort's unit (csrc/grid_records.hip): 4 record kernels (D), 3 radix kernels
UNITS = {'grid_ordered': (106, ('k_ord_sum_records', 'k_ord_sum_partials', 'k_grid_bwd_bwd', 'k_grid_input_backward'), [64, 8, 32, 2]),
         'grid_records': (7, ('k_rec_records', 'k_rec_radix'), [4, 3])}


@pytest.mark.parametrize('build,unit', [(0, 'grid_ordered'), (1, 'grid_ordered'), (0, 'grid_records'), (1, 'grid_records')],
                         ids=['product', 'debug_bounds', 'records-product', 'records-debug_bounds'])
def test_unit_has_no_scratch_no_hazard_and_no_float_atomics(build, unit, tmp_path):
    isa, objs = _objects(unit)
    n_kernels, names, counts = UNITS[unit]
    checked, hits = isa.scan_object(objs[build])
    assert checked == n_kernels and hits == []
    co = isa.code_object(objs[build], str(tmp_path))
    meta, kernels = isa.kernel_metadata(co), isa.disassembly(co)
    count = lambda s: sum(1 for k in meta if s in k)
    assert len(meta) == n_kernels
    assert [count(s) for s in names] == counts and sum(counts) == n_kernels
    assert [k for k, m in meta.items() if m['private_segment_fixed_size']] == []
    notes = subprocess.check_output([isa.TOOLS[2], '--notes', co], text=True)
    spills = re.findall(r'\.(?:s|v)gpr_spill_count:\s+(\d+)', notes)
    assert len(spills) == 2 * len(meta) and all(int(n) == 0 for n in spills)
    assert [k for k, ins in kernels.items() if any(i.startswith('scratch_') for i in ins)] == []
    assert [k for k, ins in kernels.items() if any('cmpswap' in i for i in ins)] == []
    # no float atomic anywhere, global or flat; the only atomics are the radix histogram's integer LDS adds
    for k, ins in kernels.items():
        atomics = {i.split()[0] for i in ins if 'atomic' in i}
        assert atomics == set(), (k, atomics)
        assert not any(re.match(r'(global|flat|buffer)_atomic|ds_add_(rtn_)?f|ds_pk_add', i) for i in ins), k


def test_sibling_units_keep_their_kernels():
    """the shared code moved into headers (grid_index.h, grid_second.h): the second-order unit holds its own kernel alone (the fp64 run
    sums are fp64.hip's)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    obj = os.path.join(ROOT, 'torch-ngp_amd', 'csrc', '_obj', 'grid_second.o')
    if not isa.tools_present() or not os.path.exists(obj):
        pytest.skip('grid_second.o (run __graft_entry__.build()) or the LLVM tools are missing')
    assert isa.scan_object(obj)[0] == 44
