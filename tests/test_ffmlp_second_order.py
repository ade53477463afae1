"""CPU checks of the FFMLP second order: the float64 reference of tests/ffmlp_second_cases.py against torch double autograd and against
finite differences of the oracle's first backward; the input conditions of every case the GPU tests use; the new C entries (declared,
exported, bound; host-side validation with the documented code and message, no GPU needed); the built kernels stay out of scratch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import oracle

import ffmlp_act_cases as A
import ffmlp_second_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIN, HID, NL, B = 16, 16, 3, 8
ENTRIES = ['ngp_ffmlp_backward_backward', 'ngp_ffmlp_backward_backward_workspace_bytes']


def _small(act):
    rng = np.random.default_rng(200 + act)
    w = rng.uniform(-1, 1, A.n_params(DIN, HID, NL)) * np.sqrt(3 / HID) * A.weight_scale(act)
    x = rng.uniform(-1, 1, (B, DIN))
    return x, w, rng.normal(size=(B, 16)), rng.normal(size=(B, DIN))


def _forward64(x, w, act):
    return oracle.ffmlp_forward(x, w, DIN, 16, HID, NL, activation=act, round_hidden=False, dtype=np.float64)[1]


def _t_act(x, act):
    if act == 0:
        return torch.relu(x)
    return {1: torch.exp, 2: torch.sin, 3: torch.sigmoid, 4: lambda v: 0.5 * (10 * v + torch.sqrt(100 * v * v + 4)) / 10,
            5: lambda v: torch.log(torch.exp(10 * v) + 1) / 10, 6: lambda v: v}[act](x)


def _t_factor(h, act):
    """f as a function of the stored post-activation h"""
    if act == 0:
        return (h > 0).double()
    if act == 1:
        return h
    if act == 3:
        return h * (1 - h)
    if act == 4:
        return (10 * h) ** 2 / ((10 * h) ** 2 + 1)
    if act == 5:
        return 1 - torch.exp(-10 * h)
    return torch.ones_like(h)


@pytest.mark.parametrize('act', range(7))
def test_reference_equals_torch_double_autograd(act):
    """L = sum(u * gx) with gx from an explicit statement of the first backward (f written in h, h from the forward): torch's float64
    gradients of L with respect to g, x and every matrix against reference(round_points=False), <= 1e-12 of each maximum"""
    x, w, g, u = _small(act)
    fb = _forward64(x, w, act)
    ref = S.reference(g, x, w, fb, u, DIN, HID, NL, act, False)
    tx, tg = torch.tensor(x, requires_grad=True), torch.tensor(g, requires_grad=True)
    mats = [torch.tensor(np.array(m), requires_grad=True) for m in oracle.ffmlp_split_weights(w, DIN, 16, HID, NL)]
    h = [tx]
    for l in range(NL):
        h.append(_t_act(h[-1] @ mats[l].T, act))
    assert np.abs(h[NL].detach().numpy() - fb[NL - 1]).max() < 1e-12
    e = tg @ mats[NL]
    for l in range(NL, 0, -1):
        e = (e * _t_factor(h[l], act)) @ mats[l - 1]
    got = torch.autograd.grad((torch.tensor(u) * e).sum(), [tg, tx] + mats, allow_unused=True)
    got = [np.zeros(t.shape) if v is None else v.numpy() for v, t in zip(got, [tg, tx] + mats)]
    want = [ref['dg'], ref['dx']] + A.split(ref['gw'], DIN, HID, NL)
    for name, a, b in zip(['dg', 'dx'] + [f'W{l}' for l in range(NL + 1)], got, want):
        scale = np.abs(b).max()
        err = np.abs(a - b).max() / scale if scale > 0 else np.abs(a).max()
        print(f'act {act} {name}: {err:.2e}')
        assert err <= 1e-12, (name, err)
    if act not in S.SLOPED:
        assert not ref['dx'].any()


@pytest.mark.parametrize('act', [1, 3, 4, 5, 6])
def test_reference_agrees_with_finite_differences_along_u(act):
    """phi(g, x, w) = sum(u * grad_inputs) of oracle.ffmlp_backward(round_hidden=False) on the float64 forward: central differences along
    random directions in g, x and w against the reference's dL/dg, dL/dx, dL/dW.  Bar 1e-6 of |directional derivative| (eps 1e-5: the
    truncation term is O(eps^2), the cancellation term ~1e-16 / eps)."""
    x, w, g, u = _small(act)

    def phi(g_, x_, w_):
        gx, _ = oracle.ffmlp_backward(g_, x_, w_, _forward64(x_, w_, act), DIN, 16, HID, NL, round_hidden=False, activation=act)
        return float((u * gx).sum())

    ref = S.reference(g, x, w, _forward64(x, w, act), u, DIN, HID, NL, act, False)
    rng = np.random.default_rng(7)
    eps = 1e-5
    for name, shape, grad in (('g', g.shape, ref['dg']), ('x', x.shape, ref['dx']), ('w', w.shape, ref['gw'])):
        v = rng.normal(size=shape)
        dv = [v if n == name else 0.0 for n in 'gxw']
        fd = (phi(g + eps * dv[0], x + eps * dv[1], w + eps * dv[2]) - phi(g - eps * dv[0], x - eps * dv[1], w - eps * dv[2])) / (2 * eps)
        an = float((grad * v).sum())
        scale = float(np.abs(grad * v).sum())
        print(f'act {act} d/d{name}: fd {fd:.6e} reference {an:.6e}')
        assert abs(fd - an) <= 1e-6 * scale, (name, fd, an)


@pytest.mark.parametrize('case,B', [(c, b) for c in S.CASES for b in S.BATCHES] + [(S.MODULE_CASE, S.MODULE_B)],
                         ids=lambda v: '-'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_case_meets_its_conditions(case, B):
    din, hid, nl, act = case
    c = S.case(din, hid, nl, act, B)
    S.check_conditions(c, din, hid, nl, act)
    print(f'{case} B={B}: kg {c["kg"]} ku {c["ku"]} rounding sensitivity {c["sens"]}')
    # a raised bar is at most twice the case's rounding sensitivity
    for key, bar in S.EXTRA_BARS.get(case + (B,), {}).items():
        assert bar <= 2 * c['sens'][key]


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
    assert capi.lib.ngp_ffmlp_backward_backward.argtypes == capi._SIGNATURES['ngp_ffmlp_backward_backward']
    assert len(capi._SIGNATURES['ngp_ffmlp_backward_backward']) == 17
    assert capi.lib.ngp_ffmlp_backward_backward_workspace_bytes.restype == ctypes.c_size_t
    assert len(capi.lib.ngp_ffmlp_backward_backward_workspace_bytes.argtypes) == 5


def test_workspace_query():
    import _ngp_capi as capi
    ws = lambda B, din=32, hid=64, nl=3, act=5: int(capi.lib.ngp_ffmlp_backward_backward_workspace_bytes(B, din, hid, nl, act))
    assert ws(0) == 0
    slabs = 2 * 64 * A.n_params(32, 64, 3) * 4
    layers = 3 * 128 * 64 * 2
    assert ws(128) == 4 * layers + slabs          # d, p, q, s
    assert ws(128, act=0) == ws(128, act=2) == ws(128, act=6) == 2 * layers + slabs   # d, p
    assert ws(256) - ws(128) == 4 * layers


def _call(lib, B=128, din=32, dout=16, hid=64, nl=3, act=5, ptrs=None, outs=None, ws=ctypes.c_void_p(256), nbytes=1 << 40):
    one = ctypes.c_void_p(256)
    p = [one] * 5 if ptrs is None else ptrs
    o = [one] * 3 if outs is None else outs
    return lib.ngp_ffmlp_backward_backward(p[0], p[1], p[2], p[3], p[4], B, din, dout, hid, nl, act, o[0], o[1], o[2], ws, nbytes, None)


def test_host_validation():
    """every refusal comes before any device work: the pointers below are never dereferenced"""
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)
    err = lambda: lib.ngp_last_error()
    for i in range(5):   # grad, inputs, weights, forward_buffer, u
        p = [one] * 5
        p[i] = None
        assert _call(lib, ptrs=p) == 1 and b'ffmlp_backward_backward: NULL tensor' in err(), i
    need = int(lib.ngp_ffmlp_backward_backward_workspace_bytes(128, 32, 64, 3, 5))
    assert _call(lib, nbytes=need - 1) == 1 and b'needs a workspace of %d bytes' % need in err()
    assert _call(lib, ws=None) == 1 and b'needs a workspace' in err()
    assert _call(lib, ws=ctypes.c_void_p(256 + 64)) == 1 and b'256-byte aligned' in err()
    assert _call(lib, B=100) == 1 and b'ffmlp_backward_backward' in err() and b'128' in err()
    assert _call(lib, dout=8) == 1 and b'output_dim' in err()
    assert _call(lib, hid=48) == 1 and b'hidden_dim' in err()
    assert _call(lib, din=24) == 1 and b'input_dim' in err()
    assert _call(lib, nl=1) == 1 and b'num_layers' in err()
    assert _call(lib, act=7) == 1 and b'activation' in err()
    with pytest.raises(RuntimeError, match='ffmlp_backward_backward'):
        capi.check(_call(lib, act=7))
    # an empty batch and a call without outputs are no-ops
    assert _call(lib, B=0, ptrs=[None] * 5) == 0
    assert _call(lib, outs=[None] * 3) == 0


def test_new_kernels_use_no_scratch():
    """k_ffmlp_tangent_layered and k_ffmlp_dgrad2_layered for all five widths, product and debug-bounds build: no private memory, no
    spills (tests/test_isa_invariants.py holds every kernel of the unit to the same; this names the new ones)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_isa_hazards as isa
    objs = [os.path.join(ROOT, 'torch-ngp_amd', 'csrc', d, 'ffmlp.o') for d in ('_obj', '_obj_dbg')]
    if not isa.tools_present() or not all(os.path.exists(o) for o in objs):
        pytest.skip('ffmlp.o (run __graft_entry__.build()) or the LLVM tools are missing')
    import tempfile
    for obj in objs:
        with tempfile.TemporaryDirectory() as d:
            meta = isa.kernel_metadata(isa.code_object(obj, d))
        new = {k: m for k, m in meta.items() if 'k_ffmlp_tangent_layered' in k or 'k_ffmlp_dgrad2_layered' in k}
        assert len(new) == 10, sorted(new)
        assert [k for k, m in new.items() if m['private_segment_fixed_size']] == []
