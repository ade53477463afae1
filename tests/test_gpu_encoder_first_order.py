"""GPU checks of the SH and frequency encoders' first-order kernels -- ngp_sh_encode_forward / _backward in fp32, fp16 and fp64
(csrc/shencoder.hip, the SH pair of csrc/fp64.hip), ngp_freq_encode_forward / _backward (csrc/freqencoder.hip) -- through the bindings,
against the float64 definitions, the cases and the criteria of tests/encoder_first_cases.py (tests/test_encoder_first_cases.py proves on
the CPU that the float32 twin and independent stand-in kernels meet every criterion and that every deliberately wrong variant fails one).

Every output buffer has 64 guard rows behind row B and is prefilled with a NaN bit pattern, the SH backward finds a non-zero prior in
grad_inputs (it accumulates) and runs twice, the frequency backward finds the sentinel (it overwrites); the backward models are evaluated
from the GPU's own stored dy_dx / outputs.  Every test prints its report (criterion, observed figure, bar) before it asserts (pytest -s).

A frequency backward with D = 3 would need B > 5.6 M rows and about 1.4 GB per buffer to send its grid-stride loop on a second trip; the
second trip of that kernel is taken with D = 64 instead (TRIP_BACKWARD).

MEASURED on the MI355X (kernel error beside its bar; worst over the batch sizes unless B is given).  No kernel missed a bar, nothing in
csrc/ was changed.
    fp32 SH, worst column in units of its bound   values 0.17 / 0.17 / 0.20 / 0.26 / 0.32 / 0.36 / 0.54 / 0.59 for degree 1 .. 8 (column bounds
                                                  8.7e-8 .. 9.0e-5), dy_dx 0 / 0.09 / 0.20 / 0.20 / 0.41 / 0.59 / 0.67 / 0.73 (bounds up to 3.3e-4);
                                                  the 45 identically zero derivative columns hold exact zeros.  The library is built with
                                                  -ffp-contract=off: the figures of degree 8 are those of the float32 Horner evaluation
                                                  without fused multiply-adds in test_encoder_first_cases (0.590 / 0.733)
    fp16 SH                                       every output between the roundings of def -/+ bound; at degree 8, B = 1000: 55 of 64000 values
                                                  and 100 of 192000 derivatives are not the nearest fp16 of the definition, the farthest
                                                  definition 0.069 of the bound from the rounding tie; both bindings give the same bits
    fp64 SH                                       at most 0.0094 of the rel-1e-12 rule (values), 0.0054 (dy_dx), 0.0064 (grad_inputs)
    SH backward fp32 (B = 1000)                   degree 2: 1.2e-7 (bar 7.8e-7), 4: 7.9e-7 (3.4e-6), 6: 2.6e-6 (2.6e-5), 8: 2.7e-5 (1.7e-4); the
                                                  float32 model's own error at degree 8 is 2.7e-5
    SH backward fp16                              at degree 8, B = 1000: 4 of 3000 sums are not the nearest fp16, 0.003 of the bound from the tie
    frequency sines                               6.9e-8 at most, the second trip included (bar 3e-7)
    frequency backward (B = 1000)                 (3,4) 2.7e-6 (bar 1.4e-5), (3,10) 1.4e-4 (7.5e-4), (2,6) 1.0e-5 (5.3e-5), (1,1) 2.6e-7 (1.5e-6),
                                                  (64,1) 3.8e-7 (2.1e-6), (3,0) 0 (a copy: exact); second trip (64,1), B = 262145: 6.8e-7 (3.6e-6).
                                                  The kernel's error equals the float32 model's to three digits in every case
    guard rows                                    intact in every case
"""
import numpy as np
import pytest
import torch

import encoder_first_cases as E

pytestmark = pytest.mark.gpu


def _sh_backend(binding):
    if binding == 'ctypes':
        from shencoder.backend import _backend
        return _backend
    import _shencoder
    return _shencoder


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check(rep, what):
    print(f'\n{what}\n{rep}')
    assert not rep.failures(), (what, rep.failures())


def _sh_case(backend, B, kind, degree):
    """forward with dy_dx, forward without, the backward twice on a non-zero prior and once on zeros -> (Report, dict of the host copies of
    every buffer)"""
    N = degree * degree
    x = cu(E.sh_dirs(B, kind))
    out, dy, lone = cu(E.guarded(B, N, kind)), cu(E.guarded(B, 3 * N, kind)), cu(E.guarded(B, N, kind))
    backend.sh_encode_forward(x, out, B, 3, degree, dy)
    backend.sh_encode_forward(x, lone, B, 3, degree, None)
    got = dict(outputs=host(out), dy_dx=host(dy), lone=host(lone))
    rep = E.sh_forward_criteria(got, B, kind, degree)
    rep.add('outputs without dy_dx: same bits', np.array_equal(_bits(got['lone']), _bits(got['outputs'])), '', 'bit-equal')
    grad, prior = E.sh_grad(B, kind, degree)
    buf = E.guarded(B, 3, kind)
    buf[:B] = prior
    g, gi = cu(grad), cu(buf)
    backend.sh_encode_backward(g, x, B, 3, degree, dy, gi)
    got['once'] = host(gi)
    backend.sh_encode_backward(g, x, B, 3, degree, dy, gi)
    got['twice'] = host(gi)
    rep += E.sh_backward_criteria(got['once'], prior, grad, got['dy_dx'], B, kind)
    rep += [(name + ' (second call)',) + tuple(rest) for name, *rest in E.sh_backward_criteria(got['twice'], got['once'][:B], grad, got['dy_dx'], B, kind)]
    buf[:B] = 0
    gz = cu(buf)
    backend.sh_encode_backward(g, x, B, 3, degree, dy, gz)
    got['from_zero'] = host(gz)
    rep.add('prior shows in the result', not np.array_equal(_bits(got['from_zero'][:B]), _bits(got['once'][:B])), '', 'differs from a zero-prior call')
    return E.Report(rep), got


@pytest.mark.parametrize('kind', ['f32', 'f16', 'f64'])
@pytest.mark.parametrize('degree', E.SH_DEGREES)
def test_sh_kernels_against_the_float64_definition(degree, kind):
    """every batch size of SH_BATCHES: values and dy_dx per column, the call without dy_dx bit-equal, the guard rows behind a partial wave
    intact, grad_inputs accumulated onto a non-zero prior over two calls.  The fp16 instantiations run through the ctypes binding and
    through the compiled module: the same bits."""
    worst = {}
    for B in E.SH_BATCHES:
        rep, got = _sh_case(_sh_backend('ctypes'), B, kind, degree)
        for name, ok, fig, *_ in rep:
            if isinstance(fig, float):
                worst[name] = max(worst.get(name, 0.0), fig)
        if rep.failures() or B == 1000:
            print(f'\nSH {kind} degree {degree} B={B}\n{rep}')
        assert not rep.failures(), (B, rep.failures())
        if kind == 'f16':
            rep2, got2 = _sh_case(_sh_backend('compiled'), B, kind, degree)
            assert not rep2.failures(), (B, rep2.failures())
            for k in got:
                assert np.array_equal(_bits(got[k]), _bits(got2[k])), (B, k)
    print(f'SH {kind} degree {degree}: worst figures over B in {E.SH_BATCHES}: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))


def test_sh_module_accumulates_grad_over_two_calls():
    """SHEncoder(degree=4) twice on the same leaf: the module zero-fills grad_inputs for the accumulating kernel, autograd adds the two
    results -- .grad after the first backward meets the backward criterion on a zero prior, after the second it is exactly its double"""
    from shencoder import SHEncoder
    B, degree, kind = 257, 4, 'f32'
    enc = SHEncoder(degree=degree)
    x = cu(E.sh_dirs(B, kind)).requires_grad_(True)
    grad, _ = E.sh_grad(B, kind, degree)
    w = cu(grad)
    (enc(x) * w).sum().backward()
    first = x.grad.detach().clone()
    (enc(x) * w).sum().backward()
    second = x.grad.detach().clone()
    dy = cu(E.guarded(B, 3 * degree * degree, kind))
    _sh_backend('ctypes').sh_encode_forward(x.detach(), cu(E.guarded(B, degree * degree, kind)), B, 3, degree, dy)
    buf = E.guarded(B, 3, kind)
    buf[:B] = host(first)
    _check(E.sh_backward_criteria(buf, np.zeros((B, 3), np.float32), grad, host(dy), B, kind), 'SHEncoder(degree=4).grad after one backward')
    assert torch.equal(second, first + first) and bool((first != 0).all())


@pytest.mark.parametrize('D,deg', E.FREQ_SHAPES)
def test_frequency_kernels_against_the_float64_definition(D, deg):
    """every batch size of FREQ_BATCHES: identity block exact, sines within 3e-7 of the float64 sine of the fp32 argument, grad_inputs
    (which held the sentinel: the entry overwrites) within the yardstick of the float32 model on the GPU's stored outputs, guard rows intact"""
    from freqencoder.backend import _backend as Fq
    C = D + 2 * D * deg
    for B in E.FREQ_BATCHES:
        x, grad = E.freq_case(D, deg, B)
        out, gi = cu(E.guarded(B, C, 'f32')), cu(E.guarded(B, D, 'f32'))
        Fq.freq_encode_forward(cu(x), B, D, deg, C, out)
        Fq.freq_encode_backward(cu(grad), out, B, D, deg, C, gi)
        stored = host(out)
        rep = E.Report(E.freq_forward_criteria(stored, x, deg) + E.freq_backward_criteria(host(gi), grad, stored, D, deg))
        _check(rep, f'frequency D={D} deg={deg} B={B}')


def test_frequency_forward_second_trip_through_the_grid():
    """B * C = 65536 * 256 + 62: the first 62 lanes of workgroup 0 go round the grid-stride loop a second time, at t >= 2^24"""
    from freqencoder.backend import _backend as Fq
    D, deg, B = E.TRIP_FORWARD
    C = D + 2 * D * deg
    x, _ = E.freq_case(D, deg, B)
    out = cu(E.guarded(B, C, 'f32'))
    Fq.freq_encode_forward(cu(x), B, D, deg, C, out)
    _check(E.freq_forward_criteria(host(out), x, deg), f'frequency forward D={D} deg={deg} B={B}')


def test_frequency_backward_second_trip_through_the_grid():
    """B * D = 65536 * 256 + 64 with D = 64: the last row is written on the second trip"""
    from freqencoder.backend import _backend as Fq
    D, deg, B = E.TRIP_BACKWARD
    C = D + 2 * D * deg
    x, grad = E.freq_case(D, deg, B)
    out, gi = cu(E.guarded(B, C, 'f32')), cu(E.guarded(B, D, 'f32'))
    Fq.freq_encode_forward(cu(x), B, D, deg, C, out)
    Fq.freq_encode_backward(cu(grad), out, B, D, deg, C, gi)
    stored = host(out)
    assert E.sentinel_count(stored[:B], 'f32') == 0 and E.sentinel_count(stored[B:], 'f32') == E.GUARD * C
    _check(E.freq_backward_criteria(host(gi), grad, stored, D, deg), f'frequency backward D={D} deg={deg} B={B}')
