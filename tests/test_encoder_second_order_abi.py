"""CPU checks of the frequency / SH encoders' second-order entry points and the fp64 frequency encoder (include/ngp_hip.h
ngp_freq_encode_forward_f64, ngp_freq_encode_backward_f64, ngp_freq_encode_backward_backward, ngp_sh_encode_backward_backward): declared,
exported and bound; the ABI version unchanged; host-side validation (documented codes and messages, no GPU needed); the new unit's built
objects (no scratch, no spills, no last-register 64-bit shift, no atomics); the generator reproduces the five committed tables; the
generated Hessian tables against autograd's second derivative of the basis polynomials."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from encoder_second_cases import ROOT, gen_sh, sh_reference, unit_vectors

CSRC = os.path.join(ROOT, 'torch-ngp_amd', 'csrc')
ENTRIES = {'ngp_freq_encode_forward_f64': 7, 'ngp_freq_encode_backward_f64': 8, 'ngp_freq_encode_backward_backward': 11,
           'ngp_sh_encode_backward_backward': 11}


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name, n_args in ENTRIES.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        assert getattr(capi.lib, name).argtypes == capi._SIGNATURES[name] and len(capi._SIGNATURES[name]) == n_args
        # each entry's comment names the reference function it extends
        comment = text[:text.index('int ' + name + '(')].rsplit('/*', 1)[1]
        assert re.search(r'(freq|sh)_encode_(forward|backward) \((freq|sh)encoder\.cu:\d+-\d+\)', comment), name


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_compiled_modules_gain_no_public_names():
    """the Python packages reach the new entries through _ngp_capi (tests/test_bindings.py pins the compiled modules' tables)"""
    import freqencoder.freq as fq
    import shencoder.sphere_harmonics as sh
    assert callable(fq.freq_encode_backward_backward) and callable(sh.sh_encode_backward_backward)
    for mod, names in ((fq, ('freq_encode_forward', 'freq_encode_backward')), (sh, ('sh_encode_forward', 'sh_encode_backward'))):
        public = sorted(n for n in dir(mod._backend) if not n.startswith('_') and 'encode' in n)
        assert public == sorted(names), public


ONE = ctypes.c_void_p(256)


def _freq2(lib, B=8, D=3, deg=4, C=27, dtype=0, ptrs=None):
    p = [ONE] * 5 if ptrs is None else ptrs
    return lib.ngp_freq_encode_backward_backward(p[0], p[1], p[2], B, D, deg, C, p[3], p[4], dtype, None)


def _sh2(lib, B=8, D=3, C=4, dtype=0, ptrs=None):
    p = [ONE] * 6 if ptrs is None else ptrs
    return lib.ngp_sh_encode_backward_backward(p[0], p[1], p[2], p[3], B, D, C, p[4], p[5], dtype, None)


def test_host_validation():
    import _ngp_capi as capi
    lib, F16, F32, F64 = capi.lib, capi.NGP_F16, capi.NGP_F32, capi.NGP_F64
    err = lambda: lib.ngp_last_error()
    # --- fp64 frequency forward / first backward: check_freq's messages, NULL tensors, B == 0
    assert lib.ngp_freq_encode_forward_f64(ONE, 4, 3, 2, 16, ONE, None) == 1
    assert b'freq_encode_forward_f64: output_dim must be input_dim + 2 * input_dim * degree (got 16 for D=3, degree=2)' in err()
    assert lib.ngp_freq_encode_forward_f64(ONE, 4, 0, 2, 0, ONE, None) == 1 and b'input dim must be positive' in err()
    assert lib.ngp_freq_encode_forward_f64(None, 4, 3, 2, 15, ONE, None) == 1 and b'freq_encode_forward_f64: NULL tensor' in err()
    assert lib.ngp_freq_encode_forward_f64(ONE, 4, 3, 2, 15, None, None) == 1 and b'NULL tensor' in err()
    assert lib.ngp_freq_encode_forward_f64(None, 0, 3, 2, 15, None, None) == 0
    assert lib.ngp_freq_encode_backward_f64(ONE, ONE, 4, 3, 2, 16, ONE, None) == 1
    assert b'freq_encode_backward_f64: output_dim must be input_dim + 2 * input_dim * degree' in err()
    for i in range(3):
        p = [ONE] * 3
        p[i] = None
        assert lib.ngp_freq_encode_backward_f64(p[0], p[1], 4, 3, 2, 15, p[2], None) == 1 and b'freq_encode_backward_f64: NULL tensor' in err(), i
    assert lib.ngp_freq_encode_backward_f64(None, None, 0, 3, 2, 15, None, None) == 0
    # --- frequency, second order
    assert _freq2(lib, C=28) == 1
    assert b'freq_encode_backward_backward: output_dim must be input_dim + 2 * input_dim * degree (got 28 for D=3, degree=4)' in err()
    assert _freq2(lib, D=0, C=0) == 1 and b'input dim must be positive' in err()
    for code in (F16, 7):
        assert _freq2(lib, dtype=code) == 1 and b'freq_encode_backward_backward: second order is provided for float32 and float64' in err()
    for i in range(3):   # grad, outputs, u are always needed; the two outputs are optional
        p = [ONE] * 5
        p[i] = None
        for code in (F32, F64):
            assert _freq2(lib, ptrs=p, dtype=code) == 1 and b'freq_encode_backward_backward: NULL tensor' in err(), i
    for code in (F32, F64):
        assert _freq2(lib, B=0, ptrs=[None] * 5, dtype=code) == 0
        assert _freq2(lib, ptrs=[ONE, ONE, ONE, None, None], dtype=code) == 0   # nothing asked for: nothing launched
    assert _freq2(lib, B=0, C=28) == 1   # validation comes first
    # --- SH, second order
    assert _sh2(lib, D=2) == 1 and b'sh_encode_backward_backward: SH encoder only support input dim == 3 (got 2)' in err()
    for C in (0, 9):
        assert _sh2(lib, C=C) == 1 and b'sh_encode_backward_backward: SH encoder only supports degree in [1, 8]' in err()
    for code in (F16, 7):
        assert _sh2(lib, dtype=code) == 1 and b'sh_encode_backward_backward: second order is provided for float32 and float64' in err()
    for i in range(4):   # grad, inputs, dy_dx, u
        p = [ONE] * 6
        p[i] = None
        for code in (F32, F64):
            assert _sh2(lib, ptrs=p, dtype=code) == 1 and b'sh_encode_backward_backward: NULL tensor' in err(), i
    for code in (F32, F64):
        assert _sh2(lib, B=0, ptrs=[None] * 6, dtype=code) == 0
        assert _sh2(lib, ptrs=[ONE] * 4 + [None, None], dtype=code) == 0
    assert _sh2(lib, B=0, D=4) == 1


def _objects():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    objs = [os.path.join(CSRC, d, 'encoder_second.o') for d in ('_obj', '_obj_dbg')]
    if not isa.tools_present() or not all(os.path.exists(o) for o in objs):
        pytest.skip('encoder_second.o (run __graft_entry__.build()) or the LLVM tools are missing')
    return isa, objs


@pytest.mark.parametrize('build', [0, 1], ids=['product', 'debug_bounds'])
def test_unit_has_no_scratch_no_spill_no_hazard_and_no_atomics(build, tmp_path):
    isa, objs = _objects()
    checked, hits = isa.scan_object(objs[build])
    # fp64 frequency forward / backward; the frequency second order and its wide-row form, fp32 and fp64; SH dL/dg, fp32 and fp64; SH dL/dx
    # for degrees 3..8, fp32 and fp64 (degrees 1 and 2 have no Hessian: a zero fill)
    assert checked == 2 + 4 + 2 + 12 and hits == []
    co = isa.code_object(objs[build], str(tmp_path))
    meta, kernels = isa.kernel_metadata(co), isa.disassembly(co)
    assert len(meta) == 20 and sum('k_sh_bwd_bwd_x' in k for k in meta) == 12
    assert [k for k, m in meta.items() if m['private_segment_fixed_size']] == []
    notes = subprocess.check_output([isa.TOOLS[2], '--notes', co], text=True)
    spills = re.findall(r'\.(?:s|v)gpr_spill_count:\s+(\d+)', notes)
    assert len(spills) == 2 * len(meta) and all(int(n) == 0 for n in spills)
    assert [k for k, ins in kernels.items() if any(i.startswith('global_atomic') for i in ins)] == []


def test_generator_reproduces_the_committed_tables(tmp_path):
    pytest.importorskip('sympy')
    files = ['oracle/sh_table.inc'] + ['torch-ngp_amd/csrc/' + n for n in ('sh_poly.inc', 'sh_poly64.inc', 'sh_hess.inc', 'sh_hess64.inc')]
    for f in files:
        os.makedirs(os.path.join(str(tmp_path), os.path.dirname(f)), exist_ok=True)
    gen_sh().main(str(tmp_path))
    for f in files:
        assert open(os.path.join(str(tmp_path), f), 'rb').read() == open(os.path.join(ROOT, f), 'rb').read(), f


HOST_COPY = r'''
#include "sh_hess64.inc"
/* H[i][XX, XY, XZ, YY, YZ, ZZ] of the 64 basis polynomials; entries the table leaves out are zero */
void sh_hess64_eval(double x, double y, double z, double *H) {
    for (int k = 0; k < 64 * 6; k++) H[k] = 0.0;
#define SH_HXX(i, v) H[(i) * 6 + 0] = (v)
#define SH_HXY(i, v) H[(i) * 6 + 1] = (v)
#define SH_HXZ(i, v) H[(i) * 6 + 2] = (v)
#define SH_HYY(i, v) H[(i) * 6 + 3] = (v)
#define SH_HYZ(i, v) H[(i) * 6 + 4] = (v)
#define SH_HZZ(i, v) H[(i) * 6 + 5] = (v)
    SH64_BAND_0_HESS; SH64_BAND_1_HESS; SH64_BAND_2_HESS; SH64_BAND_3_HESS;
    SH64_BAND_4_HESS; SH64_BAND_5_HESS; SH64_BAND_6_HESS; SH64_BAND_7_HESS;
}
'''


def test_hessian_table_matches_autograd_of_the_basis(tmp_path):
    """the double table (sh_hess64.inc; sh_hess.inc is the same text with float literals, see the generator test) compiled for the host,
    against autograd's second derivative of the lambdified gen_sh.basis() at unit vectors: 1e-12 of the largest of the nine second
    derivatives of that polynomial at that point (fp64 Horner forms of degree <= 5; measured 2e-13)"""
    pytest.importorskip('sympy')
    import torch
    src, so = os.path.join(str(tmp_path), 'sh_hess_host.c'), os.path.join(str(tmp_path), 'libsh_hess_host.so')
    open(src, 'w').write(HOST_COPY)
    subprocess.check_call([os.environ.get('CC', 'gcc'), '-O2', '-fPIC', '-shared', '-std=c11', '-ffp-contract=off', '-fno-fast-math', '-I', CSRC,
                           '-o', so, src])
    fn = ctypes.CDLL(so).sh_hess64_eval
    fn.argtypes = [ctypes.c_double] * 3 + [ctypes.c_void_p]
    p = unit_vectors(6, seed=11).requires_grad_(True)
    Y = sh_reference(p, 8)
    want = torch.zeros(6, 64, 3, 3, dtype=torch.float64)
    for i in range(64):
        (g,) = torch.autograd.grad(Y[:, i].sum(), p, create_graph=True, allow_unused=True)
        if g is None or not g.requires_grad:
            continue
        for d in range(3):
            (h,) = torch.autograd.grad(g[:, d].sum(), p, retain_graph=True, allow_unused=True)
            if h is not None:
                want[:, i, d] = h
    got = torch.zeros(6, 64, 6, dtype=torch.float64)
    for n in range(6):
        fn(*[float(v) for v in p[n].tolist()], got[n].data_ptr())
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    worst = 0.0
    for k, (a, b) in enumerate(pairs):
        assert torch.equal(want[:, :, a, b], want[:, :, b, a]) or torch.allclose(want[:, :, a, b], want[:, :, b, a], rtol=0, atol=1e-12)
        scale = want.abs().amax(dim=(2, 3))
        err = (got[:, :, k] - want[:, :, a, b]).abs()
        assert bool(((scale > 0) | (err == 0)).all())    # constant and linear polynomials: exactly zero
        worst = max(worst, float((err / scale.clamp_min(1e-300)).max()))
    print(f'largest Hessian error relative to the row maximum: {worst:.3g}')
    assert worst <= 1e-12
    assert float(want[:, 4:].abs().amax()) > 1.0   # (the reference is not vacuous)
