"""CPU checks of tests/render_features_cases.py, the model and tables tests/test_gpu_render_features.py holds the feature compositor of the
inference loop to (k_composite_rays_feat): the float32 model IS render_loop_cases.composite_model on the colour and on the
weight channel, bit for bit; it composites the samples the compositor's definition composites; fp32 and fp64 take the same branches on every
table; the NaN rows behind a ray's break never reach `out`; the two classic mistakes of a compositor leave the bound."""
import numpy as np
import pytest

import render_features_cases as F
import render_loop_cases as L


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_float32_model_on_the_colours_has_the_bits_of_the_compositors_image(n_step):
    t = L.composite_table(n_step)
    want = L.run_model(t, np.float32)
    out, count = F.features_model(t, t['rgbs'], t['image'], np.float32)
    assert out.dtype == np.float32 and np.array_equal(_bits(out), _bits(want['image']))
    assert np.array_equal(count, want['count'])
    ref, _ = F.features_model(t, t['rgbs'], t['image'], np.float64)
    assert np.array_equal(_bits(ref), _bits(L.table_reference(n_step)['image']))


@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_float32_model_on_a_ones_channel_has_the_bits_of_weights_sum(n_step):
    t = L.composite_table(n_step)
    want = L.run_model(t, np.float32)
    ones = np.ones((L.N_ALIVE, n_step, 1), np.float32)
    out, _ = F.features_model(t, ones, t['weights_sum'][:, None], np.float32)
    assert np.array_equal(_bits(out[:, 0]), _bits(want['weights_sum']))
    assert not np.array_equal(out[:, 0], t['weights_sum'])


@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_tables_counts_poison_and_bounds(n_step):
    want = L.table_reference(n_step)['count']
    assert want.min() == 0 and want.max() == n_step
    for C in F.CHANNELS_CPU:
        t = F.features_table(n_step, C)
        assert t['feats'].shape == (L.N_ALIVE, n_step, C) and t['out0'].shape == (L.N, C) and t['feats'].dtype == np.float32
        assert np.abs(t['out0']).min() >= 0.1
        poisoned = np.isnan(t['feats']).all(-1)
        assert np.array_equal(poisoned.sum(1), n_step - want) and np.array_equal(np.isnan(t['feats']).any(-1), poisoned)
        if n_step > 1:
            assert poisoned.any()
        ref, count64 = F.features_reference(n_step, C)
        f32, count32 = F.features_model(t, t['feats'], t['out0'], np.float32)
        e2, count_e2 = F.features_model(t, t['feats'], t['out0'], np.float32, exp2=True)
        assert np.array_equal(count64, want) and np.array_equal(count32, want) and np.array_equal(count_e2, want)
        assert np.isfinite(ref).all() and np.isfinite(f32).all() and np.isfinite(e2).all()       # the poisoned rows were not read
        outside = t['outside']
        assert np.array_equal(_bits(f32[outside]), _bits(t['out0'][outside]))
        listed = t['rays_alive'][want > 0]
        assert (f32[listed] != t['out0'][listed]).any(-1).sum() >= 0.8 * len(listed)   # (not the transparent ray: its weights are 0; a tiny weight may round away)
        bound, err = F.features_bound(n_step, C)
        bound2, err2 = F.features_bound(n_step, C, exp2=True)
        print(f'n_step={n_step} C={C}: float32 model error {err:.3e}, bound {bound:.3e}; exp2 form {err2:.3e}, {bound2:.3e}')
        assert 0 < err < 1e-5 and 0 < err2 < 1e-5 and bound < 4.1e-5 and 0.25 * bound <= bound2 <= 4.0 * bound


@pytest.mark.parametrize('variant', L.VARIANTS[1:])
def test_tables_tell_the_classic_mistakes_from_the_definition(variant):
    """`T <= T_thresh` and the threshold test BEFORE the accumulation, restated for the channels.  Neither reads a poisoned row (both stop
    EARLIER than the definition), so what gives them away is a value outside the bound.  'le' with n_step = 1 is the one table that cannot
    tell: the ray on the threshold composites its only sample either way, and the feature kernel does not write the alive list."""
    for n_step in L.N_STEPS:
        for C in (1, 33):
            t = F.features_table(n_step, C)
            ref, _ = F.features_reference(n_step, C)
            bad, count = F.features_model(t, t['feats'], t['out0'], np.float32, variant=variant)
            assert np.isfinite(bad).all() and (count <= L.table_reference(n_step)['count']).all()
            differs = float(np.abs(bad.astype(np.float64) - ref).max()) > F.features_bound(n_step, C)[0]
            assert differs == (variant != 'le' or n_step > 1), (n_step, C)


def test_reading_behind_the_break_is_seen():
    """a model that composites one row more than the definition (the row behind the break) puts NaN into `out` on every table with room"""
    for n_step in L.N_STEPS[1:]:
        t = F.features_table(n_step, 3)
        call = dict(t, T_thresh=0.0)      # never stops on the threshold: reads on into rows behind the sample that crossed it
        out, _ = F.features_model(call, t['feats'], t['out0'], np.float32)
        assert np.isnan(out).any(), n_step


def test_three_consecutive_calls():
    calls = L.multi_call_table()
    for C in (3, 33):
        tab = F.features_multi_table(C)
        assert [a.shape for a in tab['feats']] == [(c['n_alive'], L.MULTI_N_STEP, C) for c in calls]
        ref, counts64 = F.run_features_multi(C, np.float64)
        f32, counts32 = F.run_features_multi(C, np.float32)
        assert all(np.array_equal(a, b) for a, b in zip(counts64, counts32))
        assert np.isfinite(ref).all() and np.isfinite(f32).all()
        ref2, bound, err = F.features_multi_bound(C)
        assert np.array_equal(ref, ref2) and 0 < err < 1e-5 and bound < 4.1e-5
        print(f'3 calls of n_step=4, C={C}: float32 model error {err:.3e}, bound {bound:.3e}')
    # the colours through the three feature calls: the bits of the compositor's three calls
    state, _ = L.run_multi(np.float32)
    st = {k: calls[0][k].astype(np.float32) for k in L.KEYS}
    out = st['image'].copy()
    for call in calls:
        cur = dict(call, **st)
        out, _ = F.features_model(cur, call['rgbs'], out, np.float32)
        done = L.run_model(cur, np.float32)
        st = {k: done[k] for k in L.KEYS}
    assert np.array_equal(_bits(out), _bits(state['image']))
