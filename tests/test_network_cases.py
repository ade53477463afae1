"""CPU checks of tests/network_cases.py, the float64 model, cases and criteria of the fused network kernels
(tests/test_gpu_network_kernels.py): the numpy restatements against the oracle, the staged definition against one straight evaluation, its
backward against a central finite difference, the conditions the cases promise, the float32 twin against EVERY criterion the GPU test
applies, and every deliberately wrong variant against them (each must fail one)."""
import numpy as np
import pytest

import network_cases as C
import oracle

CONFIGS = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 4)]          # every (nl_s, nl_c) the GPU tests use


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
def test_sh4_and_trunc_exp_restate_the_oracle():
    d = C.nominal(2, 2, 256)['dirs']
    ref = oracle.sh_forward(d, 4).astype(np.float64)
    assert np.abs(C.sh4(d, np.float64) - ref).max() < 4e-6            # non-normalised rows reach |SH| ~ 30: a few fp32 ulps there
    assert np.abs(C.sh4(d, np.float32).astype(np.float64) - ref).max() < 4e-6
    x = np.array([-np.inf, -20.0, -15.0, -1.0, 0.0, 3.5, 15.0, 16.0, 80.0, np.nan])
    g = np.linspace(-2.0, 2.0, len(x))
    with np.errstate(over='ignore', invalid='ignore'):
        fwd = C.mid_forward(np.pad(x[:, None], ((0, 0), (0, 15))), np.zeros((len(x), 3)), len(x), 1.0)['sigma']
        np.testing.assert_allclose(fwd, oracle.trunc_exp_forward(x), rtol=1e-6)
        bwd = C.mid_backward(g, np.pad(x[:, None], ((0, 0), (0, 15))), None, 1.0, pre=True)
        np.testing.assert_allclose(bwd, oracle.trunc_exp_backward(g, x), rtol=1e-6)
    assert np.isnan(bwd[-1]) and np.isnan(oracle.trunc_exp_backward(g, x)[-1])          # the reference's clamp propagates a NaN


def test_layouts():
    x = np.arange(128 * 32, dtype=np.float64).reshape(128, 32)
    pl = C.to_planar(x)
    assert pl.shape == (16, 128, 2) and pl[3, 17, 1] == x[17, 7] and np.array_equal(C.to_rows(pl), x)


def test_staged_definition_equals_one_straight_evaluation():
    """oracle.ffmlp_forward -> trunc_exp / SH / shuffle -> oracle.ffmlp_forward -> sigmoid, written out once more with the oracle's own
    pieces: the same values up to the fp16 rounding of an SH component that the fp32 oracle and the float64 polynomial put on two sides
    of a tie"""
    case = C.nominal(2, 3, 256)
    got = C.run_forward(case, np.float64, planar=True)
    rows = C.run_forward(case, np.float64, planar=False)
    assert all(np.array_equal(got[k], rows[k]) for k in got)              # both layouts of enc are the same input
    out, _ = oracle.ffmlp_forward(case['enc'], case['w_sigma'], 32, 16, 64, 2, dtype=np.float64)
    h = oracle.round_fp16(out).astype(np.float64)
    assert np.array_equal(h, got['h16'])
    sigma = np.float32(C.DS_FORWARD) * oracle.trunc_exp_forward(h[:, 0])
    np.testing.assert_allclose(got['sigma'], sigma, rtol=3e-7)
    d = np.zeros((256, 3), np.float32)
    d[:case['M_valid']] = case['dirs']
    cin = np.concatenate([oracle.round_fp16(oracle.sh_forward(d, 4)), h[:, 1:], np.zeros((256, 1))], 1)
    diff = got['color_in'] != cin
    assert diff[:, 16:].sum() == 0 and diff.mean() < 1e-3 and np.abs(got['color_in'] - cin).max() <= 2.0 ** -10 * np.abs(cin).max()
    out, _ = oracle.ffmlp_forward(got['color_in'], case['w_color'], 32, 16, 64, 3, dtype=np.float64)
    o16 = oracle.round_fp16(out).astype(np.float64)
    rgb = oracle.round_fp16(1.0 / (1.0 + np.exp(-o16[:, :3])))
    assert np.array_equal(rgb, got['rgb'])


def test_backward_matches_a_central_difference_of_the_unrounded_forward():
    """64 rows, no rounding anywhere (round_hidden=False, the glue stages before their rounding): the directional derivative of
    L = sum(g_sigma * sigma) + sum(g_rgb * rgb) along 6 random directions in (enc, w_sigma, w_color) against the central difference with
    step 1e-7.  Truncation is O(step^2) and cancellation ~ 1e-16 / step = 1e-9 of L's scale (seen: under 8e-10 at this step, 1e-10 at
    1e-6, 6e-8 at 1e-8); a ReLU unit whose pre-activation lies within the perturbation of 0 makes the central difference average two
    slopes (seen once in six directions at step 1e-6: 6e-6; the directions are fixed by the seed, none has such a unit at 1e-7).
    Bar: 1e-7 relative to the sum of the three gradient parts' magnitudes."""
    case = C.nominal(2, 2, 128)
    n = 64
    enc, ws, wc = case['enc'][:n].astype(np.float64), case['w_sigma'].astype(np.float64), case['w_color'].astype(np.float64)
    d = case['dirs'][:n].astype(np.float64)
    rng = np.random.default_rng(3)
    g_sigma, g_rgb = rng.normal(size=n), rng.normal(size=(n, 3))
    ds = C.DS_BACKWARD

    def forward(enc, ws, wc):
        h, fb_s = oracle.ffmlp_forward(enc, ws, 32, 16, 64, 2, round_hidden=False, dtype=np.float64)
        sigma = np.float64(np.float32(ds)) * np.exp(h[:, 0])
        cin = np.concatenate([C.sh4(d), h[:, 1:], np.zeros((n, 1))], 1)
        out, fb_c = oracle.ffmlp_forward(cin, wc, 32, 16, 64, 2, round_hidden=False, dtype=np.float64)
        rgb = C.rgb_forward(out, pre=True)
        return (g_sigma * sigma).sum() + (g_rgb * rgb).sum(), (h, fb_s, cin, fb_c, rgb)

    _, (h, fb_s, cin, fb_c, rgb) = forward(enc, ws, wc)
    assert np.abs(h[:, 0]).max() < 15                                        # the clamp is inactive: trunc_exp's backward is exp's
    g_out = np.concatenate([C.rgb_backward(g_rgb, rgb, pre=True), np.zeros((n, 13))], 1)
    g_cin, g_wc = oracle.ffmlp_backward(g_out, cin, wc, fb_c, 32, 16, 64, 2, round_hidden=False)
    g_h = np.concatenate([C.mid_backward(g_sigma, h, None, ds, pre=True)[:, None], g_cin[:, 16:31]], 1)
    g_enc, g_ws = oracle.ffmlp_backward(g_h, enc, ws, fb_s, 32, 16, 64, 2, round_hidden=False)
    step = 1e-7
    for _ in range(6):
        v_e, v_s, v_c = rng.normal(size=enc.shape), rng.normal(size=ws.shape), rng.normal(size=wc.shape)
        fd = (forward(enc + step * v_e, ws + step * v_s, wc + step * v_c)[0] - forward(enc - step * v_e, ws - step * v_s, wc - step * v_c)[0]) / (2 * step)
        parts = [(g_enc * v_e).sum(), (g_ws * v_s).sum(), (g_wc * v_c).sum()]
        assert abs(fd - sum(parts)) <= 1e-7 * sum(abs(x) for x in parts), (fd, parts)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def test_nominal_case_has_the_stated_layout():
    c = C.nominal(2, 3, 256)
    for k in ('enc', 'w_sigma', 'w_color', 'g_out16'):
        assert np.array_equal(c[k], oracle.round_fp16(c[k])), k
    assert c['M_valid'] == 256 - 37 and c['dirs'].shape == (219, 3) and (c['g_out16'] != 0).all()
    norm = np.linalg.norm(c['dirs'].astype(np.float64), axis=1)
    assert (np.abs(norm - 1) > 1e-3).sum() == 64 + 4 and (norm == 0).sum() == 4 and (np.abs(c['dirs']).max(1) == 1).sum() >= 8
    assert np.abs(c['enc']).max() <= 0.5 and np.abs(c['w_sigma']).max() <= (3 / 64) ** 0.5 + 1e-3
    assert np.array_equal(C.nominal(2, 3, 128)['enc'], c['enc'][:128])
    assert abs(c['g_sigma'].std() / 1e-3 - 1) < 0.2 and abs(c['g_out16'].std() / 0.05 - 1) < 0.2


@pytest.mark.parametrize('nl_s', [2, 3, 4])
def test_wide_h0_conditions_hold(nl_s):
    """at least 2 % of the rows below -15 and above 15, every h0 < 80, |column 0 of g_h16| < 65504 -- at every M the GPU tests may use; and,
    with column 0 scaled by 2**-shift, fp16-finite hidden gradients in the sigma net's backward (which the unscaled column overflows)"""
    nl_c = min(nl_s, 3)
    for M in C.WIDE_M:
        w = C.wide_conditions(C.wide_h0(nl_s, nl_c, M), backward=M in (128, 4224))
        assert w['below'] >= 0.02 and w['above'] >= 0.02 and w['h0_max'] < 80 and w['g0_max'] < 65504, (M, w)
        if 'hidden_max' in w:
            assert w['hidden_max'] < 65504 / 16, (M, w)
            seed, power, shift = C.WIDE[nl_s]
            assert w['g0_max'] * (3 / 64) ** 0.5 * 2.0 ** power > 65504      # ... what the shift is for
    w_n, w_w = C.nominal(nl_s, nl_c, 128)['w_sigma'], C.wide_h0(nl_s, nl_c, 128)['w_sigma']
    assert np.array_equal(w_w, oracle.round_fp16(w_w)) and np.abs(w_w[-1024:-960]).max() > 16 * np.abs(w_n).max()


def test_glue_table_holds_the_stated_rows():
    t = C.glue_table()
    h0 = t['h16'][:, 0]
    for v in C.H0_VALUES:
        rows = np.isnan(h0) if np.isnan(v) else (h0 == v) & (np.signbit(h0) == np.signbit(v))
        assert set(t['g_sigma'][rows].tolist()) == set(np.float32(C.G_SIGMA_VALUES).tolist()), v
    for c in range(3):
        col = t['out16'][:, c]
        for v in C.OUT_VALUES:
            rows = np.isnan(col) if np.isnan(v) else col == v
            assert len(set(t['g_rgb'][rows, c].tolist())) == len(C.G_RGB_VALUES), (c, v)
    assert {65504.0, -65504.0, np.inf, -np.inf, 17.0, -17.0, 8.0, -8.0, 0.0, 2.0 ** -24} <= set(C.OUT_VALUES) and any(np.isnan(C.OUT_VALUES))
    assert len({tuple(r) for r in t['h16'][:, 1:]}) == t['M'] and np.array_equal(t['h16'][5, 1:], 5 + np.arange(1, 16) / 16)
    ref = C.run_glue(t, np.float64)
    assert np.isinf(ref['g_h16'][:, 0]).any() and np.isinf(ref['g_out16'][:, :3]).any()          # products that overflow fp16
    assert (np.abs(t['g_sigma'][t['g_sigma'] != 0]).min() < 2.0 ** -126) and (t['g_sigma'] == 0).any() and (t['g_rgb'] == 0).any()
    assert C.tiled_table(257)['h16'].shape == (257, 16)


def test_mse_and_pad_cases():
    assert sorted({c['n'] for c in C.mse_cases()}) == [1, 63, 64, 1023, 1024, 1025, 3 * 4099] and {c['scale'] for c in C.mse_cases()} == {None, 1024.0}
    for case in C.mse_cases():
        ref, g64 = C.mse_model(case['image'], case['target'], case['scale'], np.float64)
        f32, g32 = C.mse_model(case['image'], case['target'], case['scale'], np.float32)
        bound, err = C.yardstick('loss', case)
        assert abs(f32 - ref) == err and bound < 2e-6 * ref and g32.dtype == np.float32
        np.testing.assert_allclose(g32, g64, rtol=3e-7)
    shapes = [a for a, _, _ in C.pad_cases()]
    assert any(st > sc for _, sc, st, _, _ in shapes) and any(sr == 0 for sr, *_ in shapes) and any((sr, sc) == (dr, dc) for sr, sc, _, dr, dc in shapes)
    assert any((dr * dc) % 256 for *_, dr, dc in shapes)
    for (sr, sc, st, dr, dc), src, want in C.pad_cases():
        assert want.shape == (dr, dc) and (want[:sr, :sc] != 0).all() and want[sr:].sum() == 0 and want[:, sc:].sum() == 0


# ---- the criteria --------------------------------------------------------------------------------------------------------------------------
def _all_reports(case, dtype, variant=None):
    with np.errstate(all='ignore'):
        fwd = C.run_forward(case, dtype, variant)
        bwd = C.run_backward(case, fwd, dtype, variant)
        return C.forward_criteria(fwd, case) + C.backward_criteria(bwd, fwd, case)


def _table_report(dtype, variant=None, rows=None):
    with np.errstate(all='ignore'):
        t = C.glue_table() if rows is None else C.tiled_table(rows)
        return C.glue_criteria(C.run_glue(t, dtype, variant), t)


@pytest.mark.parametrize('kind', ['nominal', 'wide_h0'])
@pytest.mark.parametrize('nl_s,nl_c', CONFIGS)
def test_float32_twin_meets_every_gpu_criterion(nl_s, nl_c, kind):
    """the reference alone stays within every cap: the float32 model of the same statements, chained like the GPU launches (its own h16
    feeds its mid stage, ...), against the float64 definition evaluated from the twin's stored tensors"""
    rep = _all_reports(C.CASES[kind](nl_s, nl_c, 4224), np.float32)
    print(f'\n{kind} ({nl_s},{nl_c})\n{C.Report(rep)}')
    assert not C.Report(rep).failures()
    assert len(rep) == 16


def test_float32_twin_meets_the_table_criteria():
    for rows in (None, 257):
        rep = _table_report(np.float32, rows=rows)
        print(f'\n{rep}')
        assert not rep.failures() and len(rep) == 10


def test_definition_meets_its_own_criteria():
    for kind in C.CASES:
        assert not C.Report(_all_reports(C.CASES[kind](2, 3, 128), np.float64)).failures()
    assert not _table_report(np.float64).failures()


# variant -> a criterion that must reject it (the named test of tests/test_gpu_network_kernels.py that applies it is in the comment)
REJECTED_BY = {
    'clamp at 16': 'g_h16[:,0]',                                    # test_fused_backward_against_the_float64_model[wide_h0], test_glue_kernels_on_the_table
    'no clamp': 'g_h16[:,0]',                                       # the same
    'NaN h0 -> exp(-15)': 'table g_h16[:,0]',                       # test_glue_kernels_on_the_table, test_backward_epilogue_on_the_table
    'density_scale dropped in the backward': 'g_h16[:,0]',          # test_fused_backward_against_the_float64_model
    'features h[:,0:15]': 'feature shuffle',                        # test_fused_forward_against_the_float64_model
    'pad column non-zero': 'zero pad',                              # the same
    'SH halves swapped': 'SH block',                                # the same
    'planar input read as row-major': 'h16[:,1:16]',                # test_fused_forward_against_the_float64_model[PLANAR]
    'planar dL/dx written row-major': 'g_enc (planar)',             # test_fused_backward_against_the_float64_model
    'rgb not rounded to fp16': 'rgb == half(rgb)',                  # test_fused_forward_against_the_float64_model
    'tail rows use the last valid direction': 'SH(0) behind M_valid',   # the same
}


@pytest.mark.parametrize('variant', C.WRONG_VARIANTS)
def test_every_wrong_variant_is_rejected(variant):
    """each deliberately wrong model, at float64 (no rounding noise to hide behind), fails the criterion named in REJECTED_BY on the smallest
    cases the GPU tests use (M = 128) or on the table"""
    assert set(REJECTED_BY) == set(C.WRONG_VARIANTS)
    failed = set()
    for kind in C.CASES:
        failed |= {r[0] for r in C.Report(_all_reports(C.CASES[kind](2, 2, 128), np.float64, variant)).failures()}
    failed |= {r[0] for r in _table_report(np.float64, variant).failures()}
    print(variant, '->', sorted(failed))
    assert REJECTED_BY[variant] in failed, failed
