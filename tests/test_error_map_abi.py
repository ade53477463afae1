"""CPU checks of the error-map entries (ngp_error_map_draw / ngp_error_map_update, csrc/error_map.hip): declared, exported and bound with
matching argtypes at ABI 11, listed in INTEGRATION.md, ctypes-only; every documented refusal comes back before any device work; and the
instruction-level invariants tests/test_isa_invariants.py keeps for the older units hold for the new one."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import check_isa_hazards as isa  # noqa: E402

NAMES = ('ngp_error_map_draw', 'ngp_error_map_update')


def _header():
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    raw, code = _header()
    assert capi.lib.ngp_abi_version() == 11 and capi.ABI_VERSION == 11   # additive entries: the ABI version stays
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    want = {'ngp_error_map_draw': [vp, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp],
            'ngp_error_map_update': [vp, vp, vp, vp, u32, u32, f32, f32, vp]}
    for name in NAMES:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', code, flags=re.S)
        assert m, f'{name} is not declared in include/ngp_hip.h'
        assert len(m.group(1).split(',')) == len(want[name])
        fn = getattr(capi.lib, name)
        assert list(fn.argtypes) == want[name] and fn.restype is ctypes.c_int
        assert name in capi.EXPORTED
    # each declaration cites the reference lines it replaces
    assert re.search(r'get_rays \(nerf/utils\.py:\d+.*?int ngp_error_map_draw', raw, flags=re.S)
    assert re.search(r'Trainer\'s error-map update \(nerf/utils\.py.*?int ngp_error_map_update', raw, flags=re.S)
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    bindings = open(os.path.join(ROOT, 'torch-ngp_amd', 'csrc', 'bindings.cpp')).read()
    for name in NAMES:
        assert name in integration, f'{name} is missing from INTEGRATION.md'
        assert name not in bindings and 'error_map' not in bindings   # ctypes-only: the reference's pybind tables stay as they are
    assert 'error_map.hip' in open(os.path.join(ROOT, 'torch-ngp_amd', 'csrc', 'Makefile')).read()


def test_draw_refusals_need_no_gpu():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first

    def draw(em=one, B=1, res=128, N=4096, H=800, W=800, inds=one, coarse=one):
        return lib.ngp_error_map_draw(em, B, res, N, H, W, 0, None, inds, coarse, None, None, None)

    for kw in (dict(em=None), dict(inds=None), dict(coarse=None)):
        assert draw(**kw) == 1 and b'NULL' in lib.ngp_last_error()
    for res in (0, 129, 4096):
        assert draw(res=res, N=0) == 1 and b'res' in lib.ngp_last_error()
    assert draw(N=128 * 128 + 1) == 1 and b'without replacement' in lib.ngp_last_error()
    assert draw(res=3, N=10) == 1
    for H, W in ((0, 800), (800, 0), (1 << 16, 1 << 15), (0xffffffff, 0xffffffff)):
        assert draw(H=H, W=W) == 1 and b'H * W' in lib.ngp_last_error()
    with pytest.raises(RuntimeError, match='error_map_draw'):
        capi.check(draw(res=0))
    # nothing to do: no launch, no device needed
    assert draw(B=0) == 0 and draw(N=0) == 0
    assert draw(H=46340, W=46340, B=0) == 0   # H * W just below 2^31 is accepted


def test_update_refusals_need_no_gpu():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(16)
    for k in range(4):
        args = [one, one, one, one]
        args[k] = None
        assert lib.ngp_error_map_update(*args, 8, 64, 0.1, 0.9, None) == 1 and b'NULL' in lib.ngp_last_error()
    assert lib.ngp_error_map_update(one, one, one, one, 0, 64, 0.1, 0.9, None) == 0


def test_python_surface_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from nerf import utils
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        utils.draw_error_map(torch.ones(1, 64), 8, 8, 4, seed=1, res=8)
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        utils.get_rays(torch.eye(4)[None], (1.0, 1.0, 0.5, 0.5), 8, 8, N=4, error_map=torch.ones(1, 64), seed=1, res=8)
    with pytest.raises(ValueError):
        utils.ErrorMaps(2, 'cpu', res=129)
    assert hasattr(utils.ErrorMaps, 'draw') and hasattr(utils.ErrorMaps, 'update')


@pytest.mark.parametrize('build', ['_obj', '_obj_dbg'])
def test_error_map_kernels_do_not_spill_and_hold_no_hazardous_shift(build, tmp_path):
    """what tests/test_isa_invariants.py asserts per compiled unit, for csrc/error_map.hip: no scratch (the 16 keys per lane stay in
    registers), and no 64-bit shift whose amount sits in the last allocated VGPR (tools/check_isa_hazards.py)"""
    obj = os.path.join(ROOT, 'torch-ngp_amd', 'csrc', build, 'error_map.o')
    if not os.path.exists(obj) or not isa.tools_present():
        pytest.skip(f'{obj} (run __graft_entry__.build()) or the LLVM tools are missing')
    meta = isa.kernel_metadata(isa.code_object(obj, str(tmp_path)))
    kernels = {k: v for k, v in meta.items() if 'k_error_map' in k}
    assert len(kernels) == 2, sorted(meta)
    for sym, m in kernels.items():
        assert m['private_segment_fixed_size'] == 0, f'{sym}: {m["private_segment_fixed_size"]} bytes of scratch per lane'
    checked, hits = isa.scan_object(obj)
    assert checked >= 2 and not hits, hits[:4]
