"""CPU checks of the grid encoder's second-order entry points (include/ngp_hip.h ngp_grid_encode_backward_backward and its workspace
query): declared, exported and bound; the ABI version unchanged; host-side validation (documented codes and messages, no GPU needed); the
new unit's built objects (no scratch, no spills, no last-register 64-bit shift, float atomics without compare-and-swap loops)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['ngp_grid_encode_backward_backward', 'ngp_grid_backward_backward_workspace_bytes']


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
    assert capi.lib.ngp_grid_encode_backward_backward.argtypes == capi._SIGNATURES['ngp_grid_encode_backward_backward']
    assert len(capi._SIGNATURES['ngp_grid_encode_backward_backward']) == 21
    assert capi.lib.ngp_grid_backward_backward_workspace_bytes.restype == ctypes.c_size_t


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_workspace_query():
    import _ngp_capi as capi
    lib = capi.lib
    ws = lambda B, D=3, dtype=capi.NGP_F64, L=16: int(lib.ngp_grid_backward_backward_workspace_bytes(None, B, D, 2, L, dtype))
    # fp64: the record sort of the first-order fp64 backward, one level at a time (B and D alone)
    for B, D in ((1 << 18, 3), (1000, 5), (7, 2)):
        assert ws(B, D) == int(lib.ngp_grid_backward_workspace_bytes(None, B, D, 2, 16, 1.0, 16, 0, 0, capi.NGP_F64)) > 0
    assert ws(0) == 0 and ws(64, L=0) == 0 and ws(64, D=6) == 0
    # fp16 / fp32 scatter with atomics: no scratch
    assert ws(1 << 18, dtype=capi.NGP_F32) == 0 and ws(1 << 18, dtype=capi.NGP_F16) == 0


def _call(lib, B=8, D=3, C=2, L=2, dtype=0, ptrs=None, ws=None, nbytes=0):
    one = ctypes.c_void_p(256)
    p = [one] * 8 if ptrs is None else ptrs
    return lib.ngp_grid_encode_backward_backward(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], B, D, C, L, 1.0, 4, 0, 0, 0, dtype, ws, nbytes,
                                                 None)


def test_host_validation():
    import _ngp_capi as capi
    lib, F16, F32, F64 = capi.lib, capi.NGP_F16, capi.NGP_F32, capi.NGP_F64
    one = ctypes.c_void_p(256)
    err = lambda: lib.ngp_last_error()
    assert _call(lib, D=6) == 1 and b'grid_encode_backward_backward' in err() and b'input dim' in err()
    assert _call(lib, D=1) == 1 and b'input dim' in err()
    assert _call(lib, C=3) == 1 and b'C must be 1, 2, 4, or 8' in err()
    assert _call(lib, L=0) == 1 and b'number of levels' in err()
    assert _call(lib, L=33) == 1 and b'number of levels' in err()
    assert _call(lib, dtype=7) == 1 and b'float32, float16 or float64' in err()
    assert _call(lib, C=1, dtype=F16) == 1 and b'float16 tables need an even C' in err()
    # NULL tensors: the six inputs that are always needed; grad_grad and grad_inputs2 are optional outputs
    for i in (0, 1, 2, 3, 4, 6):
        p = [one] * 8
        p[i] = None
        assert _call(lib, ptrs=p) == 1 and b'NULL tensor' in err(), i
    # B == 0 is a no-op, whatever the pointers
    assert _call(lib, B=0, ptrs=[None] * 8) == 0
    assert _call(lib, B=0, ptrs=[None] * 8, dtype=F64) == 0
    # fp64: the record limit, the workspace size and its alignment
    assert _call(lib, B=1 << 27, D=5, dtype=F64, ws=one, nbytes=1 << 40) == 1 and b'2^31' in err()
    assert _call(lib, dtype=F64) == 1 and b'fp64 needs a workspace' in err()
    need = int(lib.ngp_grid_backward_backward_workspace_bytes(None, 8, 3, 2, 2, F64))
    assert _call(lib, dtype=F64, ws=one, nbytes=need - 1) == 1 and b'fp64 needs a workspace of %d bytes' % need in err()
    assert _call(lib, dtype=F64, ws=ctypes.c_void_p(256 + 64), nbytes=need) == 1 and b'256-byte aligned' in err()
    # fp32 / fp16 take no workspace (the checks above come before any device work)
    assert _call(lib, C=3, dtype=F32) == 1


def _objects():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    objs = [os.path.join(ROOT, 'torch-ngp_amd', 'csrc', d, 'grid_second.o') for d in ('_obj', '_obj_dbg')]
    if not isa.tools_present() or not all(os.path.exists(o) for o in objs):
        pytest.skip('grid_second.o (run __graft_entry__.build()) or the LLVM tools are missing')
    return isa, objs


@pytest.mark.parametrize('build', [0, 1], ids=['product', 'debug_bounds'])
def test_unit_has_no_scratch_no_hazard_and_plain_float_atomics(build, tmp_path):
    isa, objs = _objects()
    checked, hits = isa.scan_object(objs[build])
    assert checked == 44 and hits == []
    co = isa.code_object(objs[build], str(tmp_path))
    meta, kernels = isa.kernel_metadata(co), isa.disassembly(co)
    # 16 (D, C) shapes for fp32 and fp64, 12 for fp16 (even C); the fp64 run sums are fp64.hip's (tests/test_fp64_abi.py)
    assert len(meta) == 44 and all('k_grid_bwd_bwd' in k for k in meta)
    assert [k for k, m in meta.items() if m['private_segment_fixed_size']] == []
    # no spills at all, not even into AGPRs or VGPR lanes
    notes = subprocess.check_output([isa.TOOLS[2], '--notes', co], text=True)
    spills = re.findall(r'\.(?:s|v)gpr_spill_count:\s+(\d+)', notes)
    assert len(spills) == 2 * len(meta) and all(int(n) == 0 for n in spills)
    assert [k for k, ins in kernels.items() if any(i.startswith('scratch_') for i in ins)] == []
    assert [k for k, ins in kernels.items() if any('cmpswap' in i for i in ins)] == []
    # fp32 tables: global_atomic_add_f32; fp16: global_atomic_pk_add_f16; fp64 (k_grid_bwd_bwdId...): no float atomics
    for k, ins in kernels.items():
        atomics = {i.split()[0] for i in ins if i.startswith('global_atomic')}
        if 'k_grid_bwd_bwdIf' in k:
            assert atomics == {'global_atomic_add_f32'}, k
        elif 'k_grid_bwd_bwdIDF16_' in k:
            assert atomics == {'global_atomic_pk_add_f16'}, k
        else:
            assert atomics == set(), k
