"""CPU checks of the fp64 path's boundary: NGP_F64 in the header and the bindings, the *_f64 raymarching entries exported and bound, host-side
validation of the fp64 entries (documented codes and messages, no GPU needed), the mixed-dtype errors raised before any device work, and the
fp64 unit's built objects (no scratch, no last-register 64-bit shift)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_ENTRIES = ['ngp_near_far_from_aabb_f64', 'ngp_sph_from_ray_f64', 'ngp_packbits_f64', 'ngp_composite_rays_train_forward_f64',
               'ngp_composite_rays_train_backward_f64', 'ngp_composite_rays_f64']


def test_ngp_f64_is_declared():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    assert re.search(r'\bNGP_F64\s*=\s*2\b', text)
    assert capi.NGP_F64 == 2 and capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_fp64_entries_are_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name in F64_ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and capi._SIGNATURES[name]
        assert getattr(capi.lib, name).argtypes == capi._SIGNATURES[name]


def test_grid_fp64_host_validation():
    import _ngp_capi as capi
    lib, F64 = capi.lib, capi.NGP_F64
    one = ctypes.c_void_p(256)
    # the deterministic backward's scratch: a function of B and D alone -- no host offsets needed
    ws = lambda B, D=3: int(lib.ngp_grid_backward_workspace_bytes(None, B, D, 2, 16, 1.0, 16, 0, 0, F64))
    arrays = lambda B, D: 4 * ((4 * (B << D) + 255) // 256 * 256)
    counts = (256 * 1024 + 256) * 4   # per-(digit, workgroup) counts and the digit totals of one sort pass
    assert ws(1 << 18) == arrays(1 << 18, 3) + counts
    assert ws(1000, 5) == arrays(1000, 5) + counts
    assert ws(0) == 0
    offs = (ctypes.c_int32 * 17)(*range(0, 17 * 64, 64))
    assert int(lib.ngp_grid_backward_workspace_bytes(ctypes.cast(offs, ctypes.c_void_p), 1 << 18, 3, 2, 16, 1.0, 16, 0, 0, F64)) == ws(1 << 18)
    # ... which the plain entry cannot be given, and the _ws entry checks
    rc = lib.ngp_grid_encode_backward(one, one, one, one, one, 8, 3, 2, 2, 1.0, 4, None, None, 0, 0, 0, F64, None)
    assert rc == 1 and b'fp64 needs a workspace' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_backward_ws(one, one, one, one, one, 8, 3, 2, 2, 1.0, 4, None, None, 0, 0, 0, F64, 0.0, None, one, 64, None)
    assert rc == 1 and b'fp64 needs a workspace' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_backward_ws(one, one, one, one, one, 1 << 27, 5, 2, 2, 1.0, 4, None, None, 0, 0, 0, F64, 0.0, None, one, 1 << 40, None)
    assert rc == 1 and b'2^31' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_backward_ws(one, one, one, one, one, 8, 3, 2, 2, 1.0, 4, one, None, 0, 0, 0, F64, 0.0, None, one, 1 << 30, None)
    assert rc == 1 and b'dy_dx and grad_inputs' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_backward_ws(one, one, one, one, one, 8, 3, 3, 2, 1.0, 4, None, None, 0, 0, 0, F64, 0.0, None, one, 1 << 30, None)
    assert rc == 1 and b'C must be 1, 2, 4, or 8' in lib.ngp_last_error()
    # fused, graph and optimizer entries keep refusing it
    rc = lib.ngp_grid_encode_backward_checked(one, one, one, one, one, 8, 3, 2, 2, 1.0, 4, None, None, 0, 0, 0, F64, 0.0, None, one, 1 << 30, None, None)
    assert rc == 1 and b'float64 is not provided by this entry point' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_forward_sel(one, one, None, None, None, one, one, 8, 3, 2, 2, 1.0, 4, 0, 0, 0, F64, 0.0, None, None)
    assert rc == 1 and b'float64 is not provided by this entry point' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_forward_ex(one, one, one, one, 8, 3, 2, 2, 1.0, 4, None, 0, 0, 0, F64, 1.0, None)
    assert rc == 1 and b'float64 is provided without the fused input mapping' in lib.ngp_last_error()
    # forward argument checks apply to fp64 as to the other dtypes; an unknown code keeps its message
    rc = lib.ngp_grid_encode_forward(one, one, one, one, 8, 3, 3, 2, 1.0, 4, None, 0, 0, 0, F64, None)
    assert rc == 1 and b'C must be 1, 2, 4, or 8' in lib.ngp_last_error()
    rc = lib.ngp_grid_encode_forward(one, one, one, one, 8, 3, 2, 2, 1.0, 4, None, 0, 0, 0, 7, None)
    assert rc == 1 and b'embeddings must be float32 or float16' in lib.ngp_last_error()
    assert lib.ngp_grid_encode_forward(None, None, None, None, 0, 3, 2, 2, 1.0, 4, None, 0, 0, 0, F64, None) == 0
    rc = lib.ngp_grad_total_variation(one, one, one, one, 1.0, 8, 6, 2, 2, 1.0, 4, 0, 0, F64, None)
    assert rc == 1 and b'input dim' in lib.ngp_last_error()


def test_sh_and_raymarching_fp64_host_validation():
    import _ngp_capi as capi
    lib, F64 = capi.lib, capi.NGP_F64
    one = ctypes.c_void_p(256)
    rc = lib.ngp_sh_encode_forward(one, one, 8, 3, 9, None, F64, None)
    assert rc == 1 and b'degree in [1, 8]' in lib.ngp_last_error()
    rc = lib.ngp_sh_encode_forward(one, None, 8, 3, 4, None, F64, None)
    assert rc == 1 and b'NULL tensor' in lib.ngp_last_error()
    assert lib.ngp_sh_encode_backward(None, None, 0, 3, 4, None, None, F64, None) == 0
    rc = lib.ngp_composite_rays_train_forward_f64(one, None, one, one, 16, 4, 1e-4, one, one, one, None)
    assert rc == 1 and b'composite_rays_train_forward_f64: NULL tensor' in lib.ngp_last_error()
    rc = lib.ngp_composite_rays_train_backward_f64(None, one, one, one, one, one, one, one, 16, 4, 1e-4, one, one, None)
    assert rc == 1 and b'NULL tensor' in lib.ngp_last_error()
    rc = lib.ngp_composite_rays_f64(4, 8, 1e-2, one, one, one, one, one, one, None, one, None)
    assert rc == 1 and b'composite_rays_f64: NULL tensor' in lib.ngp_last_error()
    for rc in (lib.ngp_near_far_from_aabb_f64(one, one, None, 4, 0.2, one, one, None), lib.ngp_sph_from_ray_f64(one, None, 1.0, 4, one, None),
               lib.ngp_packbits_f64(None, 4, 0.5, one, None)):
        assert rc == 1 and b'NULL tensor' in lib.ngp_last_error()
    assert lib.ngp_packbits_f64(None, 0, 0.5, None, None) == 0 and lib.ngp_composite_rays_f64(0, 8, 1e-2, *([None] * 8), None) == 0


def test_mixed_float64_calls_raise_before_device_work():
    import _ngp_capi as capi
    import _raymarching
    from raymarching.backend import _backend as rm
    d, f = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.float32)
    assert capi.float_code(d, 'x') == capi.NGP_F64 and capi.float64_call((f, 'f'), (None, 'none')) is False
    with pytest.raises(RuntimeError, match='fars must be a float64 tensor'):
        capi.float64_call((d, 'rays_o'), (f, 'fars'))
    aabb, nears = torch.ones(6, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    for backend in (rm, _raymarching):
        with pytest.raises(RuntimeError, match='fars must be a float64 tensor'):
            backend.near_far_from_aabb(d, d, aabb, 4, 0.2, nears, f)
        with pytest.raises(RuntimeError, match='CUDA tensor'):   # an all-float64 call gets as far as the device checks
            backend.near_far_from_aabb(d, d, aabb, 4, 0.2, nears, nears.clone())


def _fp64_objects():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    objs = [os.path.join(ROOT, 'torch-ngp_amd', 'csrc', d, 'fp64.o') for d in ('_obj', '_obj_dbg')]
    if not isa.tools_present() or not all(os.path.exists(o) for o in objs):
        pytest.skip('fp64.o (run __graft_entry__.build()) or the LLVM tools are missing')
    return isa, objs


@pytest.mark.parametrize('build', [0, 1], ids=['product', 'debug_bounds'])
def test_fp64_unit_has_no_scratch_and_no_last_register_shift(build, tmp_path):
    isa, objs = _fp64_objects()
    checked, hits = isa.scan_object(objs[build])
    assert checked >= 90 and hits == []
    co = isa.code_object(objs[build], str(tmp_path))
    meta, kernels = isa.kernel_metadata(co), isa.disassembly(co)
    assert len(meta) >= 90 and all(k.startswith('_ZN3ngp') and 'k_f64_' in k for k in meta)
    assert [k for k, m in meta.items() if m['private_segment_fixed_size']] == []
    assert [k for k, ins in kernels.items() if any(i.startswith('scratch_') for i in ins)] == []
    # the deterministic backward uses no float atomics; TV (not on an autograd path) adds with fp64 atomics
    atomics = {k for k, ins in kernels.items() if any(re.match(r'global_atomic_\w*f(32|64)', i) for i in ins)}
    assert atomics and all('k_f64_grad_tv' in k for k in atomics)
    # the second-order run sums (k_f64_grid_run_sum<D, C, 2>, 16 (D, C) shapes): no spills at all, not even into AGPRs or VGPR lanes, no
    # compare-and-swap and no float atomics
    second = [k for k in meta if re.search(r'k_f64_grid_run_sumILi\dELi\dELi2EE', k)]
    assert len(second) == 16 and sum(1 for k in meta if 'k_f64_grid_run_sum' in k) == 32
    notes = subprocess.check_output([isa.TOOLS[2], '--notes', co], text=True)
    seen, spilled = set(), set()
    for block in notes.split('.agpr_count:')[1:]:
        symbol = re.search(r'\.symbol:\s+(\S+)\.kd', block).group(1)
        counts = re.findall(r'\.(?:s|v)gpr_spill_count:\s+(\d+)', block)
        assert len(counts) == 2, symbol
        seen.add(symbol)
        if any(int(n) for n in counts):
            spilled.add(symbol)
    assert set(second) <= seen and not spilled & set(second)
    for k in second:
        assert not any('cmpswap' in i for i in kernels[k]), k
        assert {i.split()[0] for i in kernels[k] if i.startswith('global_atomic')} == set(), k
