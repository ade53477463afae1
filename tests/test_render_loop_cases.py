"""CPU checks of tests/render_loop_cases.py, the cases and references of the inference loop's kernels (tests/test_gpu_render_loop.py): the
float64 definition against the restated oracle, the float32 yardstick model against the reference's own kernel compiled for the host (where
oracle/_ref is built), the conditions the tables promise (no ordinary ray near T_thresh, every named ray does what its name says, the three
exact-threshold rays take the stated branch in every implementation), loop_n_step against the renderer's rule and the ladder, the compaction
table, and that the tables tell the two classic compositor mistakes from the definition."""
import numpy as np
import pytest

import oracle
import render_loop_cases as C
from oracle import ref as oref

needs_ref = pytest.mark.skipif(not oref.available('nofma'), reason='oracle/_ref not built (make -C oracle ref, needs /root/reference)')


def _within(got, ref, bounds, what):
    for key in C.KEYS:
        err = float(np.abs(np.asarray(got[key], np.float64) - ref[key]).max())
        assert err <= bounds[key][0], (what, key, err, bounds[key])


def _oracle_call(fn, call, state=None, **kw):
    """one call of an fp32-I/O implementation on a table's inputs -> dict like composite_model's"""
    s = {k: np.ascontiguousarray((state or call)[k], np.float32).copy() for k in C.KEYS}
    alive = np.ascontiguousarray(call['rays_alive'], np.int32).copy()
    sg, rg, de = call['sigmas'].reshape(-1), call['rgbs'].reshape(-1, 3), call['deltas'].reshape(-1, 2)
    if fn is oracle.composite_rays:
        alive, s['rays_t'], s['weights_sum'], s['depth'], s['image'] = fn(call['n_alive'], call['n_step'], alive, s['rays_t'], sg, rg, de,
                                                                          s['weights_sum'], s['depth'], s['image'], T_thresh=call['T_thresh'])
    else:   # in place
        fn(call['n_alive'], call['n_step'], alive, s['rays_t'], sg, rg, de, s['weights_sum'], s['depth'], s['image'], T_thresh=call['T_thresh'], **kw)
    return dict(s, rays_alive=alive)


# ---- the compositor tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_tables_have_the_stated_layout(n_step):
    t = C.composite_table(n_step)
    assert t['n_alive'] == 61 and len(t['rays_alive']) == 61 and len(t['outside']) == 36
    assert sorted(np.concatenate([t['rays_alive'], t['outside']]).tolist()) == list(range(97))
    assert t['rays_alive'].tolist() != sorted(t['rays_alive'].tolist())       # scattered ids
    assert t['sigmas'].shape == (61, n_step) and t['rgbs'].shape == (61, n_step, 3) and t['deltas'].shape == (61, n_step, 2)
    for key in C.KEYS:
        assert t[key].dtype == np.float32 and (t[key] != 0).all()             # non-zero, fp32-representable state
    ks = [int(n.split()[-1]) for n in t['names'] if n.startswith('finished at ')]
    assert ks == (list(range(n_step + 1)) if n_step <= 8 else [0, 1, n_step - 1])
    assert len(set(t['names'].values())) == len(t['names'])


@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_no_ordinary_ray_is_near_the_threshold(n_step):
    """|T / T_thresh - 1| > 1e-3 at every step of the definition, for every list entry; the three exact rays only with their FIRST sample
    excepted -- so fp32 and fp64 may not disagree on any alive-list entry"""
    t, ref = C.composite_table(n_step), C.table_reference(n_step)
    exact = {t['names'][e] for e in C.EXACT}
    for n, seen in enumerate(ref['T_seen']):
        for k, T in enumerate(seen):
            if n in exact and k == 0:
                continue
            assert abs(T / C.T_THRESH - 1.0) > C.MARGIN, (n, k, T)
    assert C.margin_violations(ref['T_seen'], exact) == []
    # the float32 model then takes the same branches: 1e-3 of T_thresh is 7.8e-6, the fp32 error of weights_sum a few 6e-8
    f32 = C.run_model(t, np.float32)
    assert np.array_equal(f32['rays_alive'], ref['rays_alive']) and np.array_equal(f32['count'], ref['count'])
    assert C.yardstick(n_step)['weights_sum'][1] < 0.1 * C.MARGIN * C.T_THRESH
    # ... and both branches are there
    assert (ref['rays_alive'] >= 0).sum() >= 5 and (ref['rays_alive'] < 0).sum() >= 5


@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_named_rays_do_what_their_names_say(n_step):
    t, ref = C.composite_table(n_step), C.table_reference(n_step)
    names, alive0, count = t['names'], t['rays_alive'], ref['count']
    dead = ref['rays_alive'] < 0
    for name, n in names.items():
        i = alive0[n]
        if name.startswith('finished at '):
            k = int(name.split()[-1])
            assert (t['deltas'][n, k:] == 0).all() and (t['deltas'][n, :k] > 0).all()
            assert count[n] == k and dead[n] == (k < n_step), name
            if k == 0:
                assert all(ref[key][i] == t[key][i] if key != 'image' else (ref[key][i] == t[key][i]).all() for key in C.KEYS)
        elif name == 'opaque':
            assert np.allclose(t['sigmas'][n].astype(np.float64) * t['deltas'][n, :, 0], 20.0, rtol=1e-6)
            assert count[n] == min(2, n_step) and dead[n] == (n_step >= 2) and ref['weights_sum'][i] > 1 - 1e-8
        elif name == 'transparent':
            assert (t['sigmas'][n] == 0).all() and count[n] == n_step and not dead[n]
            assert ref['weights_sum'][i] == t['weights_sum'][i] and ref['depth'][i] == t['depth'][i]
            assert abs(ref['rays_t'][i] - (t['rays_t'][i] + t['deltas'][n, :, 1].astype(np.float64).sum())) < 1e-12
        elif name == 'already saturated':
            assert t['weights_sum'][i] == np.float32(0.9995) and count[n] == 1 and dead[n]
            assert ref['weights_sum'][i] > t['weights_sum'][i]                # that one sample IS composited
    # a stopped ray keeps its rays_t, a continuing one moves
    for n in range(61):
        i = alive0[n]
        assert (ref['rays_t'][i] == t['rays_t'][i]) == bool(dead[n]), n
    for i in t['outside']:
        assert all(np.array_equal(ref[key][i], t[key][i].astype(np.float64)) for key in C.KEYS)


def _exact_branches(t, out, count=None):
    """the three exact-threshold rays: (a) T == T_thresh is not <, the ray goes on to its second sample; (b) one ulp below and (c) half the
    threshold stop after that sample"""
    n_step, alive0 = t['n_step'], t['rays_alive']
    a, b, c = (t['names'][e] for e in C.EXACT)
    assert (out['rays_alive'][a] >= 0) == (n_step == 1)
    assert out['rays_alive'][b] < 0 and out['rays_alive'][c] < 0
    for n in (a, b, c):   # each composites its first sample: weights_sum moves
        assert out['weights_sum'][alive0[n]] > t['weights_sum'][alive0[n]]
    if count is not None:
        assert count[a] == min(2, n_step) and count[b] == 1 and count[c] == 1
    # (a) and (b) start one fp32 ulp apart and see (almost) the same first sample: a second sample of (a) shows as a much larger weights_sum
    if n_step >= 2:
        gain = [float(out['weights_sum'][alive0[n]]) - float(t['weights_sum'][alive0[n]]) for n in (a, b)]
        assert gain[0] > 1.25 * gain[1]


@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_exact_threshold_rays_take_the_stated_branch_in_both_models_and_the_oracle(n_step):
    t = C.composite_table(n_step)
    a, b, c = (t['rays_alive'][t['names'][e]] for e in C.EXACT)
    # the inputs: T = 1 - ws0 is exact in fp32 and in fp64
    assert 1.0 - float(t['weights_sum'][a]) == C.T_THRESH and 1.0 - float(t['weights_sum'][c]) == C.T_THRESH / 2
    assert 1.0 - float(t['weights_sum'][b]) == C.T_THRESH - 2.0 ** -24 and np.float32(1) - t['weights_sum'][b] == np.float32(C.T_THRESH - 2.0 ** -24)
    for dtype in (np.float64, np.float32):
        out = C.run_model(t, dtype)
        _exact_branches(t, out, out['count'])
    out = C.run_model(t, np.float32, exp2=True)
    _exact_branches(t, out, out['count'])
    _exact_branches(t, _oracle_call(oracle.composite_rays, t))


@needs_ref
@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_exact_threshold_rays_take_the_stated_branch_in_the_reference_kernel(n_step):
    t = C.composite_table(n_step)
    for variant in ('nofma', 'fma'):
        if oref.available(variant):
            _exact_branches(t, _oracle_call(oref.composite_rays, t, variant=variant))


@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_float64_model_agrees_with_the_oracle(n_step):
    """oracle.composite_rays computes in double with fp32 I/O: agreement within fp32 rounding of the state = the yardstick bound"""
    t, ref = C.composite_table(n_step), C.table_reference(n_step)
    got = _oracle_call(oracle.composite_rays, t)
    assert np.array_equal(got['rays_alive'], ref['rays_alive'])
    _within(got, ref, C.yardstick(n_step), 'oracle')
    assert all(bound < 2e-5 for bound, _ in C.yardstick(n_step).values())     # the yardstick is an fp32-rounding-sized number, not a loose one


@needs_ref
@pytest.mark.parametrize('n_step', C.N_STEPS)
def test_float32_model_agrees_with_the_reference_kernel(n_step):
    """the reference's own kernel_composite_rays compiled for the host: pins the MODEL to the reference, not to this project's kernel"""
    t, ref = C.composite_table(n_step), C.table_reference(n_step)
    f32 = C.run_model(t, np.float32)
    for variant in ('nofma', 'fma'):
        if not oref.available(variant):
            continue
        got = _oracle_call(oref.composite_rays, t, variant=variant)
        assert np.array_equal(got['rays_alive'], ref['rays_alive']) and np.array_equal(got['rays_alive'], f32['rays_alive'])
        _within(got, ref, C.yardstick(n_step), variant)
        _within(got, {k: f32[k].astype(np.float64) for k in C.KEYS}, C.yardstick(n_step), variant + ' against the float32 model')


def test_exp2_form_of_the_yardstick_is_the_same_size():
    """the restated exponential exp2(fl32(x * log2 e)) moves the float32 model by rounding only"""
    for n_step in C.N_STEPS:
        a, b = C.yardstick(n_step), C.yardstick(n_step, exp2=True)
        for key in C.KEYS:
            assert 0.25 * a[key][0] <= b[key][0] <= 4.0 * a[key][0], (n_step, key, a[key], b[key])


@pytest.mark.parametrize('variant', C.VARIANTS[1:])
def test_tables_tell_the_classic_mistakes_from_the_definition(variant):
    """`T <= T_thresh` and the threshold test BEFORE the accumulation, applied to the model: the alive list or a value outside the yardstick
    gives each away on every table (what tests/test_gpu_render_loop.py would report for a kernel with that mistake)"""
    for n_step in C.N_STEPS:
        t, ref, bounds = C.composite_table(n_step), C.table_reference(n_step), C.yardstick(n_step)
        bad = C.run_model(t, np.float32, variant=variant)
        list_differs = not np.array_equal(bad['rays_alive'], ref['rays_alive'])
        value_differs = any(float(np.abs(bad[k].astype(np.float64) - ref[k]).max()) > bounds[k][0] for k in C.KEYS)
        if variant == 'le':
            assert list_differs == (n_step == 1), n_step      # with a second sample the ray on the threshold stops either way ...
            assert value_differs, n_step                       # ... but without having composited it (n_step 1: without moving rays_t)
        else:
            assert value_differs, n_step                       # 'already saturated' and the rays below the threshold lose their one sample


# ---- three consecutive calls ---------------------------------------------------------------------------------------------------------------
def test_multi_call_table():
    calls = C.multi_call_table()
    ref, lists, bounds = C.multi_yardstick()
    assert len(calls) == 3 and all(c['n_step'] == 4 for c in calls) and calls[0] is C.composite_table(4)
    sizes = [c['n_alive'] for c in calls]
    assert sizes[0] == 61 and sizes[0] > sizes[1] > sizes[2] > (lists[2] >= 0).sum() > 0       # rays leave in every call, some see all three
    for i in (1, 2):   # each call's list is the compacted list of the previous one
        assert np.array_equal(calls[i]['rays_alive'], lists[i - 1][lists[i - 1] >= 0])
    # no ray near the threshold in any call, so the float32 model and the oracle walk through the same lists
    state64 = {k: calls[0][k].astype(np.float64) for k in C.KEYS}
    state_orc = {k: calls[0][k] for k in C.KEYS}
    f32, lists32 = C.run_multi(np.float32)
    for i, call in enumerate(calls):
        out = C.run_model(dict(call, **state64), np.float64)
        exempt = {call['names'][e] for e in C.EXACT} if i == 0 else set()
        assert C.margin_violations(out['T_seen'], exempt) == []
        state64 = {k: out[k] for k in C.KEYS}
        got = _oracle_call(oracle.composite_rays, call, state_orc)
        state_orc = {k: got[k] for k in C.KEYS}
        assert np.array_equal(out['rays_alive'], lists[i]) and np.array_equal(lists32[i], lists[i]) and np.array_equal(got['rays_alive'], lists[i])
    _within(state_orc, ref, bounds, 'oracle, three calls')
    # a continuing ray's rays_t feeds the next call: a ray alive after all three calls moved by all twelve real deltas
    for n, i in enumerate(lists[2]):
        if i >= 0:
            moved = sum(float(c['deltas'][list(c['rays_alive']).index(i), :, 1].astype(np.float64).sum()) for c in calls)
            assert abs(ref['rays_t'][i] - (float(calls[0]['rays_t'][i]) + moved)) < 1e-12


# ---- loop_n_step ---------------------------------------------------------------------------------------------------------------------------
def test_loop_n_step_is_the_renderers_rule_at_cap_0():
    for N in (1, 7, 8, 9, 100, 4096, 640000):
        for n_alive in sorted({1, 2, 3, 7, 8, 9, N // 9 + 1, N // 8, N // 8 + 1, N // 2, N // 2 + 1, N - 1, N, N + 1, 2 * N} - {0}):
            assert C.loop_n_step(N, n_alive, 0) == max(min(N // n_alive, 8), 1), (N, n_alive)
            assert C.loop_n_step(N, n_alive, 8) == C.loop_n_step(N, n_alive, 0)
            assert C.loop_n_step(N, n_alive, 64) == max(min(N // n_alive, 64), 1)


def test_ladder():
    assert [row[:3] for row in C.LADDER] == [(4096, 4096, 0), (4096, 5000, 0), (4096, 1000, 0), (4096, 512, 0), (4096, 100, 0), (4096, 100, 64),
                                             (4096, 10, 64), (4096, 0, 0), (4096, 0, 64)]
    assert [row[3] for row in C.LADDER] == [1, 1, 4, 8, 8, 40, 64, 1, 1]
    for n_total, n_alive, cap, want in C.LADDER:
        assert C.loop_n_step(n_total, n_alive, cap) == want, (n_total, n_alive, cap)


def test_rows_used_is_the_strict_round_up():
    assert C.rows_used(10 ** 6, 512, 8) == 4096 + 128 and C.rows_used(10 ** 6, 1000, 4) == 4096 and C.rows_used(10 ** 6, 0, 1) == 128
    assert C.rows_used(801, 100, 8) == 801 and C.rows_used(64, 0, 1) == 64
    import raymarching.raymarching as rm
    for used in (0, 1, 127, 128, 129, 4096, 5000):
        assert C.rows_used(10 ** 6, used, 1) == rm._round_up_strict(used, 128)


# ---- compaction ----------------------------------------------------------------------------------------------------------------------------
def test_compaction_table():
    assert C.COMPACT_SIZES == (0, 1, 63, 64, 65, 255, 256, 257, 511, 513, 65536, 65537, 70001, 640000) and len(C.COMPACT_PATTERNS) == 9
    for n in C.COMPACT_SIZES:
        for pattern in C.COMPACT_PATTERNS:
            a, want = C.compaction_case(n, pattern)
            assert a.dtype == np.int32 and len(a) == n + 300 and (a[n:] >= 0).all()
            live = a[:n][a[:n] >= 0]
            assert np.array_equal(want, live) and len(set(live.tolist())) == len(live) and (live < n).all()
            expect = {'all alive': n, 'all dead': 0, 'alternating': (n + 1) // 2, '1 in 1000': n // 1000, 'only the first': min(n, 1),
                      'only the last': min(n, 1), 'lane 63 of every wave': n // 64, 'thread 255 of every block': n // 256}.get(pattern)
            if expect is not None:
                assert len(want) == expect, (n, pattern)
            elif n >= 63:
                assert 0.3 * n < len(want) < 0.7 * n
            if len(want) > 8:
                assert want.tolist() != sorted(want.tolist())     # order matters
    a, _ = C.compaction_case(63, 'all alive', length=2 * 63 + 7 + 400)
    assert len(a) == 2 * 63 + 7 + 400


# ---- the whole loop ------------------------------------------------------------------------------------------------------------------------
def test_loop_model():
    ref, ref64 = C.loop_model(np.float64, 0), C.loop_model(np.float64, 64)
    assert ref['t_exact'] and ref64['t_exact']
    # chunking independence holds in the definition itself: the same operations in the same order
    for key in C.KEYS[:3]:
        assert np.array_equal(ref[key], ref64[key])
    assert np.array_equal(ref['count'], ref64['count'])
    assert ref64['iterations'] < ref['iterations'] and ref['iterations'] > 8
    assert max(ref['steps'], ref64['steps']) + 3 * 64 < C.LOOP_MAX_STEPS      # the max_steps cut never binds, with the spare iterations issued
    hit = ref['count'] > 0
    assert 0.5 * C.LOOP_N < hit.sum() < C.LOOP_N and ref['count'].max() > 30
    assert (ref['weights_sum'][hit] > 0).all() and (ref['weights_sum'] > 1 - C.LOOP_T_THRESH).sum() > 100   # rays that stop on T_thresh ...
    assert ((ref['weights_sum'] < 0.9) & hit).sum() > 20                                                     # ... and rays that leave the box
    bounds = C.loop_yardstick()
    assert bounds['image'][0] < 0.1 * C.LOOP_T_THRESH and bounds['weights_sum'][1] > 0
    # fields64 is `fields` up to the last fp32 bit
    x = np.random.default_rng(0).uniform(-1, 1, (1000, 3)).astype(np.float32)
    for a, b in zip(C.fields(x), C.fields64(x)):
        assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -22 * np.abs(b).max()
