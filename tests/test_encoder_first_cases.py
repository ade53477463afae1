"""CPU checks of tests/encoder_first_cases.py, the float64 definitions, cases and criteria of the SH and frequency encoders' first-order
kernels (tests/test_gpu_encoder_first_order.py): the conditions the cases promise, the float32 twin and independent stand-in kernels
(oracle.sh_forward / oracle.sh_backward, an fp32 Horner evaluation in the kernel's own expression form, fused-multiply-add forms of the two
backward sums) against EVERY criterion the GPU test applies, and every deliberately wrong variant against them (each must fail one)."""
import functools

import numpy as np
import pytest

import encoder_first_cases as E
import oracle

KINDS = ('f32', 'f16', 'f64')


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def test_sh_cases_hold_the_stated_rows():
    assert E.SH_BATCHES == (1, 63, 64, 65, 255, 256, 257, 1000) and E.SH_DEGREES == tuple(range(1, 9))
    special = [[0, 0, 1], [1, 0, 0], [0, -1, 0], [0, 0, 0]]
    for kind in KINDS:
        for B in E.SH_BATCHES:
            d = E.sh_dirs(B, kind)
            assert d.shape == (B, 3) and d.dtype == E.KINDS[kind]
            assert d[:4].tolist() == special[:min(B, 4)]
            norm = np.linalg.norm(d.astype(np.float64), axis=1)
            k = min(B, 100) // 2
            off = np.abs(norm - 1) > 2e-3
            assert not off[max(k, 4):].any() and (k <= 4 or off[4:k].mean() > 0.9) and norm[4:].min(initial=1) > 0.19 and norm.max() < 1.51
            if kind != 'f64':
                assert np.array_equal(d.astype(np.float64), d.astype(np.float32).astype(np.float64))
        # a case is a prefix of the next larger one wherever both scale the row or both do not
        assert np.array_equal(E.sh_dirs(257, kind)[100:], E.sh_dirs(1000, kind)[100:257])
        assert len(E.yard_dirs(kind)) == sum(E.SH_BATCHES)


def test_sh_columns_are_exercised_and_fit_fp16():
    """every column that is not identically zero has a non-zero definition on the rows of every case with B >= 64 (a vacuous column would
    pass anything); 45 of the 192 derivative columns are identically zero (15 per variable); nothing overflows fp16, the backward's sums
    (after two calls) included"""
    zero = E.sh_zero_columns()
    assert zero.shape == (3, 64) and zero[:, 0].all() and zero.sum(1).tolist() == [15, 15, 15] and zero[:, 1:4].sum() == 6
    for kind in KINDS:
        for B in E.SH_BATCHES:
            Y, dY = E.sh_definition(B, kind, 8)
            if B >= 64:
                assert (np.abs(Y).max(0) > 0).all()
                assert np.array_equal(np.abs(dY).max(0) == 0, zero)
            assert not dY[:, zero].any()
        yd = E.sh_yardstick(kind)
        assert 40 < yd['max_Y'].max() < 100 and 300 < yd['max_dY'].max() < 800            # (fp16: far below 65504)
        assert np.array_equal(yd['bound_dY'] == 0, zero) and (yd['bound_Y'] > 0).all()
    for B in E.SH_BATCHES:
        grad, prior = E.sh_grad(B, 'f16', 8)
        assert (np.abs(prior.astype(np.float64)) >= 0.5).all() and grad.dtype == np.float16
        _, dY = E.sh_definition(B, 'f16', 8)
        twice = prior.astype(np.float64) + 2 * np.einsum('bi,bdi->bd', grad.astype(np.float64), dY)
        assert np.abs(twice).max() < 65504 / 4


def test_close64_is_the_rule_of_the_fp64_tests():
    from test_gpu_fp64 import _close
    rng = np.random.default_rng(1)
    want = rng.normal(size=(50, 7)) * 300
    for factor, passes in ((0.5, True), (2.0, False)):
        got = want + factor * (1e-12 * np.abs(want) + 1e-14 * np.abs(want).max())
        assert E.close64(got, want)[0] == passes
        if passes:
            _close(got, want)
        else:
            with pytest.raises(AssertionError):
                _close(got, want)


def test_frequency_cases():
    assert E.FREQ_SHAPES == ((3, 4), (3, 10), (2, 6), (1, 1), (3, 0), (64, 1)) and E.FREQ_BATCHES == (1, 64, 65, 257, 1000)
    D, deg, B = E.TRIP_FORWARD
    assert B * (D + 2 * D * deg) == E.GRID_CAP + 62 == 16777278 and (B - 1) * (D + 2 * D * deg) < E.GRID_CAP
    D, deg, B = E.TRIP_BACKWARD
    assert B * D == E.GRID_CAP + 64 == 16777280
    x, g = E.freq_case(3, 10, 1000)
    assert x.dtype == g.dtype == np.float32 and g.shape == (1000, 63) and np.abs(x).max() <= 1 and abs(x.mean()) < 0.05
    # the definition's cosine is the sine of the fp32 argument plus fp32(pi / 2), evaluated in float64 -- restated by hand
    arg = (x * np.float32(512.0) + np.float32(np.float32(3.141592653589793) / np.float32(2))).astype(np.float32)
    assert np.array_equal(oracle.freq_forward(x, 10)[:, 60:63], np.sin(arg.astype(np.float64)))


def test_guarded_buffers():
    for kind in KINDS:
        buf = E.guarded(3, 5, kind)
        assert buf.shape == (3 + E.GUARD, 5) and buf.dtype == E.KINDS[kind] and np.isnan(buf).all() and E.sentinel_count(buf, kind) == buf.size
        buf[E.GUARD + 2, 4] = 1.0
        assert E.sentinel_count(buf, kind) == buf.size - 1


# ---- the float32 twin and the stand-in kernels ---------------------------------------------------------------------------------------------
def _sh_reports(B, kind, degree, dtype=None, variant=None, fused=False):
    """forward with and without dy_dx, then the backward twice on a non-zero prior (the second call finds the first call's result), as the GPU
    test does -> Report"""
    fwd = E.run_sh_forward(B, kind, degree, dtype, variant)
    rep = E.sh_forward_criteria(fwd, B, kind, degree)
    lone = E.run_sh_forward(B, kind, degree, dtype, variant, with_grad=False)
    rep.add('outputs without dy_dx: same bits', np.array_equal(lone['outputs'].view(np.uint8), fwd['outputs'].view(np.uint8)), '', 'bit-equal')
    grad, prior = E.sh_grad(B, kind, degree)
    buf = E.guarded(B, 3, kind)
    buf[:B] = prior
    once = E.run_sh_backward(buf, grad, fwd['dy_dx'], B, kind, dtype, variant, fused)
    rep += E.sh_backward_criteria(once, prior, grad, fwd['dy_dx'], B, kind)
    twice = E.run_sh_backward(once, grad, fwd['dy_dx'], B, kind, dtype, variant, fused)
    rep += [(name + ' (second call)',) + tuple(rest) for name, *rest in E.sh_backward_criteria(twice, once[:B], grad, fwd['dy_dx'], B, kind)]
    zero = E.guarded(B, 3, kind)
    zero[:B] = 0
    from_zero = E.run_sh_backward(zero, grad, fwd['dy_dx'], B, kind, dtype, variant, fused)
    rep.add('prior shows in the result', not np.array_equal(from_zero[:B], once[:B]), '', 'differs from a zero-prior call')
    return E.Report(rep)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('degree', E.SH_DEGREES)
def test_float32_twin_meets_every_sh_criterion(degree, kind):
    """the float32 model (for f64: the definition) as an implementation, at every batch size of the GPU test"""
    for B in E.SH_BATCHES:
        rep = _sh_reports(B, kind, degree)
        if B in (1, 1000):
            print(f'\nSH twin {kind} degree {degree} B={B}\n{rep}')
        assert not rep.failures(), (B, rep.failures())
        assert len(rep) == (11 if kind == "f32" else 10)
        if kind != 'f64':
            fused = _sh_reports(B, kind, degree, fused=True)          # the kernel's own fma chain in the backward
            assert not fused.failures(), (B, fused.failures())


@functools.lru_cache(maxsize=None)
def _horner_callables():
    """the expression form of csrc/sh_poly.inc (tools/gen_sh.py::_double_code: expanded, Horner in z, y, x, factors to 17 digits)"""
    import sympy as sp
    g = E.gen_sh()
    v = (g.x, g.y, g.z)

    def lam(e):
        e = sp.expand(sp.nsimplify(e))
        e = sp.horner(e, g.z, g.y, g.x) if e.free_symbols else e
        return sp.lambdify(v, e.evalf(17), 'numpy')
    Y = g.basis()
    return tuple(lam(e) for e in Y), tuple(tuple(lam(sp.diff(e, s)) for e in Y) for s in v)


@pytest.mark.parametrize('kind', ['f32', 'f16'])
def test_stand_in_forward_kernels_pass_with_margin(kind):
    """the 4x bound is not slack by accident, and not out of reach either.  oracle.sh_forward (the polynomials in C, stored as fp32) lands
    at no more than 0.5 of the bound in every column of values and derivatives (seen: 0.18) -- a condition on the inputs, not a tolerance
    for the kernel.  A float32 evaluation WITHOUT fused multiply-adds of the Horner form the kernel is generated in passes too (seen: 0.59
    of the bound in the values, 0.74 in dy_dx).  Taken over the rows of the single case instead of yard_dirs, the B = 1 case would fail the
    latter (1.13 in dy_dx: at (0, 0, 1) the factored model is exact) -- why the yardstick is a column's figure over all rows."""
    yd = E.sh_yardstick(kind)
    hy, hd = _horner_callables()
    worst = dict(oracle=0.0, horner=0.0)
    for B in E.SH_BATCHES:
        d = E.sh_dirs(B, kind)
        Y, dY = E.sh_definition(B, kind, 8)
        oY, odY = oracle.sh_forward(d.astype(np.float32), 8, calc_grad_inputs=True)
        x, y, z = (d[:, i].astype(np.float32) for i in range(3))
        hY = E._columns(hy, x, y, z, np.float32)
        hdY = np.stack([E._columns(hd[s], x, y, z, np.float32) for s in range(3)], 1)
        for name, a, b in (('oracle', oY, odY.reshape(B, 3, 64)), ('horner', hY, hdY)):
            worst[name] = max(worst[name], float(E.column_ratios(a, Y, yd['bound_Y']).max()), float(E.column_ratios(b, dY, yd['bound_dY']).max()))
    print(f'\nstand-in kernels on {kind}-valued directions, worst column in units of its bound: {worst}')
    assert worst['oracle'] <= 0.5 and worst['horner'] <= 1.0


@pytest.mark.parametrize('degree', E.SH_DEGREES)
def test_stand_in_backward_kernel_passes_with_margin(degree):
    """oracle.sh_backward (the sum in a double, stored as fp32) added to the prior in float32: no more than 0.5 of the bound"""
    for B in E.SH_BATCHES:
        fwd = E.run_sh_forward(B, 'f32', degree)
        grad, prior = E.sh_grad(B, 'f32', degree)
        got = E.guarded(B, 3, 'f32')
        got[:B] = prior + oracle.sh_backward(grad, degree, fwd['dy_dx'][:B])
        want = E.sh_backward_model(prior, grad, fwd['dy_dx'][:B], np.float64)
        bound, _ = E.whole_yardstick(E.sh_backward_model(prior, grad, fwd['dy_dx'][:B], np.float32), want)
        assert np.abs(got[:B] - want).max() <= 0.5 * bound, (B, np.abs(got[:B] - want).max(), bound)
        assert not E.sh_backward_criteria(got, prior, grad, fwd['dy_dx'], B, 'f32').failures()


def _freq_reports(D, deg, B, dtype=np.float32, variant=None, contracted=False):
    x, grad = E.freq_case(D, deg, B)
    out = E.run_freq_forward(x, deg, dtype, variant)
    rep = E.freq_forward_criteria(out, x, deg)
    gi = E.run_freq_backward(grad, out, D, deg, dtype, variant, contracted)
    return E.Report(rep + E.freq_backward_criteria(gi, grad, out, D, deg))


# (D, deg) -> the float32 model's error of the backward on 1000 rows of x ~ U(-1, 1) as first measured with other draws than this module's:
# the figures are compared to a factor of 3
MEASURED_MODEL_ERROR = {(3, 4): 2.9e-6, (3, 10): 1.7e-4, (2, 6): 8.4e-6, (1, 1): 2.8e-7, (64, 1): 4.4e-7, (3, 0): 0.0}


@pytest.mark.parametrize('D,deg', E.FREQ_SHAPES)
def test_float32_twin_meets_every_frequency_criterion(D, deg):
    for B in E.FREQ_BATCHES:
        for contracted in (False, True):
            rep = _freq_reports(D, deg, B, contracted=contracted)
            if B == 1000:
                print(f'\nfrequency twin D={D} deg={deg} B={B} contracted={contracted}\n{rep}')
            assert not rep.failures(), (B, contracted, rep.failures())
            assert len(rep) == (5 if deg else 6)
    x, grad = E.freq_case(D, deg, 1000)
    out = E.run_freq_forward(x, deg)
    want = E.freq_backward_model(grad, out[:1000], D, deg, np.float64)
    bound, err = E.whole_yardstick(E.freq_backward_model(grad, out[:1000], D, deg, np.float32), want)
    m = MEASURED_MODEL_ERROR[(D, deg)]
    assert (err == 0 and bound == 1e-7 * np.abs(want).max()) if deg == 0 else m / 3 < err < 3 * m
    # the contracted form (one fma for the difference of products, one for the update) as a stand-in kernel: at most half the bound
    got = E.freq_backward_model(grad, out[:1000], D, deg, np.float32, contracted=True)
    assert np.abs(got - want).max() <= 0.5 * bound


def test_float32_twin_and_dropped_elements_on_the_trip_cases():
    """the two cases of more than 65536 * 256 elements: the twin passes, the twin without the elements of the second trip fails"""
    D, deg, B = E.TRIP_FORWARD
    x, _ = E.freq_case(D, deg, B)
    out = E.run_freq_forward(x, deg)
    assert not E.freq_forward_criteria(out, x, deg).failures()
    dropped = out.copy()
    dropped.reshape(-1)[E.GRID_CAP:B * (D + 2 * D * deg)] = E.guarded(0, 1, 'f32')[0, 0]
    assert np.array_equal(dropped.view(np.uint32), E.run_freq_forward(x, deg, variant='elements behind 65536 * 256 dropped').view(np.uint32))
    assert [r[0] for r in E.freq_forward_criteria(dropped, x, deg).failures()] == ['identity block', 'sines']      # (columns 1 .. 62 of the last row)
    del out, dropped
    D, deg, B = E.TRIP_BACKWARD
    x, grad = E.freq_case(D, deg, B)
    out = E.run_freq_forward(x, deg)
    gi = E.run_freq_backward(grad, out, D, deg)
    assert not E.freq_backward_criteria(gi, grad, out, D, deg).failures()
    gi = E.run_freq_backward(grad, out, D, deg, variant='elements behind 65536 * 256 dropped')
    assert E.sentinel_count(gi[:B], 'f32') == 64
    assert [r[0] for r in E.freq_backward_criteria(gi, grad, out, D, deg).failures()] == ['grad_inputs']


# ---- the wrong variants --------------------------------------------------------------------------------------------------------------------
# variant -> (a criterion that must reject it, the cases it is run on)
REJECTED_BY = {
    'backward overwrites': 'grad_inputs',
    'dy_dx laid out [B,N,3]': 'dy_dx',
    'band 3 in reversed m order': 'values',
    'last band left zero': 'values',
    'last partial wave not written': 'values',
    'fp16 truncated toward zero': 'values',
    'exact cosine': 'sines',
    'sin / cos interleaved per dimension': 'sines',
    'backward without 2^f': 'grad_inputs',
    'backward adds into grad_inputs': 'grad_inputs',
    'elements behind 65536 * 256 dropped': 'grad_inputs',
}


@pytest.mark.parametrize('variant', E.WRONG_VARIANTS)
def test_every_wrong_variant_is_rejected(variant):
    """each deliberately wrong model, evaluated in float64 (no rounding noise to hide behind), fails the criterion named in REJECTED_BY on
    the cases of the GPU test; where a variant needs a property of the case (a partial wave, band 3, fp16 storage, two frequencies, more
    than one trip) every case that has it must reject it"""
    assert set(REJECTED_BY) == set(E.WRONG_VARIANTS)
    name = REJECTED_BY[variant]

    def rejected(rep):
        return name in {r[0] for r in rep.failures()}

    if variant in E.WRONG_VARIANTS_SH:
        for kind in KINDS:
            for degree in (1, 4, 8):
                for B in E.SH_BATCHES:
                    # (B = 1 is the row (0, 0, 1), where band 3 is its own mirror image; degree 1 is one constant, which truncates to its nearest fp16)
                    applies = {'last partial wave not written': B % 64 != 0, 'band 3 in reversed m order': degree >= 4 and B > 1,
                               'fp16 truncated toward zero': kind == 'f16' and degree >= 2, 'dy_dx laid out [B,N,3]': degree >= 2}.get(variant, True)
                    rep = _sh_reports(B, kind, degree, np.float64, variant)
                    assert rejected(rep) == applies, (kind, degree, B, rep.failures())
                    if variant == 'backward overwrites':
                        assert 'prior shows in the result' in {r[0] for r in rep.failures()}
    elif variant == 'elements behind 65536 * 256 dropped':
        assert not _freq_reports(3, 4, 1000, np.float64, variant).failures()              # (one trip: nothing to drop)
        D, deg, B = E.TRIP_BACKWARD                                                       # (the forward's trip: the test above)
        x, grad = E.freq_case(D, deg, B)
        out = E.run_freq_forward(x, deg)
        assert rejected(E.freq_backward_criteria(E.run_freq_backward(grad, out, D, deg, np.float64, variant), grad, out, D, deg))
    else:
        for D, deg in E.FREQ_SHAPES:
            for B in E.FREQ_BATCHES:
                applies = {'exact cosine': deg >= 10, 'sin / cos interleaved per dimension': deg >= 1 and D >= 2,
                           'backward without 2^f': deg >= 2}.get(variant, True)
                rep = _freq_reports(D, deg, B, np.float64, variant)
                if variant == 'exact cosine' and 0 < deg < 10:
                    continue          # below deg = 10 the two cosines differ by less than the 3e-7 of the sine bar on some draws, by more on others
                assert rejected(rep) == applies, (D, deg, B, rep.failures())
