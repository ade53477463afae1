"""CPU checks of tests/optim_cases.py, the float64 model, cases and criteria of the optimizer kernels (tests/test_gpu_optim_model.py): the
definition against torch.optim.Adam in float64, the commit model against its hand-written table and against torch's GradScaler update, the
conditions the cases promise, the float32 twin against EVERY criterion the GPU test applies, and every deliberately wrong variant against them
(each must fail the criterion named in REJECTED_BY)."""
import functools

import numpy as np
import pytest
import torch

import optim_cases as C

F32, F16 = np.float32, np.float16


# ---- the definition and the commit model against PyTorch ---------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [0, 9])
def test_definition_is_torch_adam_in_float64(step):
    """would catch a definition that is not PyTorch's Adam: one standing step of torch.optim.Adam (float64, CPU) from the same p, m, v and step
    count on the unscaled gradient; the betas, eps and lr are the float32 values the kernels get.  rtol 1e-13: both are float64 evaluations
    of one formula, in slightly different operation orders"""
    el = C.path_elements('wide')
    state, rule = C.make_state(scale=128.0, step=float(step)), C.make_rule()
    ref = C.adam_step(el, state, rule, C.LRS[0])
    p = torch.nn.Parameter(torch.tensor(el['p'], dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=float(C.LRS[0]), betas=(float(C.BETA1), float(C.BETA2)), eps=float(C.EPS))
    opt.state[p] = dict(step=torch.tensor(float(step)), exp_avg=torch.tensor(el['m'], dtype=torch.float64),
                        exp_avg_sq=torch.tensor(el['v'], dtype=torch.float64))
    p.grad = torch.tensor(el['g'].astype(np.float64) / 128.0)
    opt.step()
    np.testing.assert_allclose(opt.state[p]['exp_avg'].numpy(), ref['m'], rtol=1e-13, atol=0)
    np.testing.assert_allclose(opt.state[p]['exp_avg_sq'].numpy(), ref['v'], rtol=1e-13, atol=0)
    np.testing.assert_allclose(p.detach().numpy(), ref['p'], rtol=1e-13, atol=0)         # (the update is 1e-5 .. 10 times |p|: see below)
    assert not ref['skip'] and np.abs(ref['upd']).max() > 1e-3


def test_commit_model_reproduces_the_hand_written_table():
    """would catch a model of update_scale that disagrees with the rows written by hand (and a table that lost a row the issue asks for)"""
    names = [r['name'] for r in C.COMMIT_TABLE]
    assert len(set(names)) == len(names)
    for row in C.COMMIT_TABLE:
        got = C.commit(row['state'], *row['rule'], row['flip'])
        assert C.same_bits(got, np.array(row['out'], F32)) == 0, (row['name'], got)
    states = [r['state'] for r in C.COMMIT_TABLE]
    assert {s[1] for s in states if s[0] == 1024 and s[2] == 0 and s[7] == 0} >= {2, 3, 4}           # tracker at I - 2, I - 1, I
    assert any(s[0] == 2.0 ** 127 for s in states) and any(s[0] == 2.0 ** -126 and s[2] for s in states) and any(s[0] == 0 for s in states)
    assert any(0 < s[0] < 2.0 ** -126 and not s[2] for s in states) and any(s[7] == 1 and s[0] == 1024 for s in states)
    assert {(s[5], r['flip'], bool(s[2])) for r in C.COMMIT_TABLE for s in [r['state']] if s[0] == 128} == {(q, f, k) for q in (0, 1) for f in (0, 1) for k in (False, True)}
    assert not C.scale_is_dead(2.0 ** -127) and C.scale_is_dead(2.0 ** -130) and C.scale_is_dead(0.0) and not C.scale_is_dead(2.0 ** 127)


def test_commit_model_is_gradscalers_update_where_gradscaler_defines_one():
    """would catch a commit model that is not GradScaler.update: torch's own _amp_update_scale_ (CPU) on the rows marked `gradscaler` -- scale
    and growth tracker.  The other rows (tracker already at the interval, the dead scale) are this project's extension and are not compared"""
    rows = [r for r in C.COMMIT_TABLE if r['gradscaler']]
    assert len(rows) >= 15 and not any('dead' in r['name'] for r in rows)
    for row in rows:
        s = row['state']
        scale, tracker, found = torch.tensor([s[0]], dtype=torch.float32), torch.tensor([int(s[1])], dtype=torch.int32), torch.tensor([float(s[2])])
        torch._amp_update_scale_(scale, tracker, found, float(row['rule'][0]), float(row['rule'][1]), int(row['rule'][2]))
        got = C.commit(s, *row['rule'], row['flip'])
        assert C.same_bits(scale.numpy(), got[C.SCALE:C.SCALE + 1]) == 0 and float(tracker) == got[C.TRACKER], (row['name'], scale, tracker, got)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def test_element_set_holds_the_stated_rows():
    """would catch a case set that lost what it is for: the eps rows, the tiny-v rows, opposite signs, fp16 edge values, fp32-only gradients"""
    el = C.elements()
    g, g32, m, v = el['g'].astype(np.float64), el['g32'].astype(np.float64), el['m'], el['v']
    assert np.isfinite(g).all() and (g == 0).sum() > 400 and ((g != 0) & (np.abs(g) < 6e-5)).sum() > 250 and (np.abs(g) > 64000).sum() > 250
    assert g[C.N - 2] != 0 and 1e-2 < abs(g[C.N - 2]) < 100                         # the odd tail of the N - 1 run carries an ordinary value
    for grad in (g, g32):
        assert ((v == 0) & (grad == 0) & (m != 0)).sum() > 100                      # the rows that see eps
        assert ((v > 0) & (v < 2e-28) & (grad == 0)).sum() > 100                    # v around eps^2
        assert ((grad * m < 0) & (np.abs(grad) == 2)).sum() > 90                    # opposite signs
    eps_rows = (v == 0) & (g == 0) & (m != 0)
    for step in C.STEPS:                                                            # step_size * m / eps of order 1e-4 .. 1e-2
        upd = np.abs(C.adam_step(C.path_elements('wide'), C.make_state(step=float(step)), C.make_rule(), C.LRS[0])['upd'][eps_rows])
        assert upd.min() > 5e-5 and upd.max() < 2e-2, (step, upd.min(), upd.max())
    only32 = g32 != g
    with np.errstate(over='ignore'):
        assert only32.sum() == len(range(14, C.N, 41)) and (g32[only32].astype(F16).astype(np.float64) != g32[only32]).all()
    assert C.same_bits(el['p16'], el['p'].astype(F16)) == 0 and not any(a.flags.writeable for a in el.values())


def test_twin_never_underflows_and_stays_within_four_ulp_of_the_definition():
    """would catch cases on which fp32 denormals decide (the criteria would then test the device's denormal mode, not Adam), and a twin whose
    operation order is not the definition's: m and v of the twin within 4 ulp (2^-23 of the operands' magnitude) of the float64 definition"""
    tiny = 2.0 ** -126
    worst = 0.0
    for path in ('wide', 'g32'):
        el = C.path_elements(path)
        for step in C.STEPS:
            for name, s in C.SCALARS.items():
                state, rule = C.make_state(scale=s['scale'], step=float(step), lr_mult=s['lr_mult']), C.make_rule(s['grad_mult'])
                ref, tw = C.adam_step(el, state, rule, C.LRS[0], dtype=np.float64), C.adam_step(el, state, rule, C.LRS[0], dtype=np.float32)
                inv = F32(rule['grad_mult']) / F32(s['scale'])
                g = el['g'].astype(F32) * inv
                gg = (F32(1.0) - C.BETA2) * g * g
                for a in (g, gg, (F32(1.0) - C.BETA1) * g, C.BETA1 * el['m'], C.BETA2 * el['v'], tw['m'], tw['v'], tw['upd']):
                    a = np.abs(a.astype(np.float64))
                    assert not ((a > 0) & (a < tiny)).any(), (path, step, name)
                assert ((gg == 0) == (el['g'] == 0)).all()                                                   # g * g did not underflow
                b1, b2 = np.float64(C.BETA1), np.float64(C.BETA2)
                g64 = el['g'].astype(np.float64) * (np.float64(rule['grad_mult']) / s['scale'])
                mag_m = np.abs(b1 * el['m']) + np.abs((1 - b1) * g64)
                mag_v = b2 * el['v'] + (1 - b2) * g64 * g64
                for got, want, mag in ((tw['m'], ref['m'], mag_m), (tw['v'], ref['v'], mag_v)):
                    keep = mag > 0
                    worst = max(worst, float((np.abs(got.astype(np.float64) - want)[keep] / mag[keep]).max()))
                    assert ((got == 0) == (want == 0))[~keep].all()
    print(f'worst |twin - definition| of m, v: {worst / 2.0 ** -23:.2f} ulp')
    assert worst <= 4 * 2.0 ** -23


def test_powers_underflow_where_the_cases_say():
    """would catch step counts and scalar sets that lost their point: 0.9^1000 and 0.99^30000 must underflow to 0 in fp32 (both corrections
    exactly 1), 0.99^1000 must not; every scale, lr_mult and grad_mult of the issue must be in a scalar set; the powf margin must be 2 x"""
    assert C._pow(C.BETA1, 1000.0, np.float32) == 0 and C._pow(C.BETA2, 30000.0, np.float32) == 0 and C._pow(C.BETA2, 1000.0, np.float32) > 4e-5
    assert C._pow(C.BETA1, 1.0, np.float32) == C.BETA1 and C.POWF_REL_ERR == 2 * C.POWF_MEASURED_REL_ERR
    assert {s['scale'] for s in C.SCALARS.values()} == {128.0, 65536.0, 3072.0} and {s['lr_mult'] for s in C.SCALARS.values()} == {1.0, 0.37}
    assert {s['grad_mult'] for s in C.SCALARS.values()} == {1.0, 1.0 / 3.0} and C.STEPS == (0, 1, 9, 999, 29999)


def test_check_and_shard_cases_hold_the_stated_plants():
    """would catch CHECK cases that lost a position (body / tail / second trip / every slot / every non-finite class) and shard layouts that
    lost the lane boundary"""
    tensors = C.check_tensors()
    assert [(len(t), t.dtype == F16) for t in tensors] == list(C.CHECK_TENSORS) and {n % 8 for n, h in C.CHECK_TENSORS if h} >= {0, 1, 7}
    assert C.check_finite(tensors, C.make_state())[C.FOUND_INF] == 0
    assert any((t == 65504).any() and (t == -65504).any() and ((t != 0) & (np.abs(t) < 6e-5)).any() for t in tensors if t.dtype == F16)
    plants = C.check_plants()
    assert {k for _, k, _, _ in plants} == set(range(8)) and {str(v) for *_, v in plants} == {'inf', '-inf', 'nan'}
    assert any(not C.CHECK_TENSORS[k][1] and e >= C.CHECK_LANES for _, k, e, _ in plants)                    # reached in the second trip only
    total = sum(n for n, _ in C.CHECK_TENSORS)
    assert C.CHECK_LANES == 256 * -(-(total // 2 + 1) // 1024) and all(n // 8 <= C.CHECK_LANES for n, h in C.CHECK_TENSORS if h)
    for name, k, e, val in plants:
        bad = [t.copy() for t in tensors]
        bad[k][e] = val
        assert C.check_finite(bad, C.make_state())[C.FOUND_INF] == 1, name
    assert C.SHARDS == (1, 2, 64, 65) and C.PAYLOADS == (1, 8, 1000) and len(C.shard_cases()) == 24
    flat = C.shard_pattern(65, 8)
    assert (flat[8:16] == 0).all() and (np.delete(flat, np.arange(8, 16)) != 0).all() and np.array_equal(flat.astype(np.float64)[:3], [1, 1.125, 1.25])


# ---- the criteria -------------------------------------------------------------------------------------------------------------------------
def _step_cases():
    for path in C.PATHS:
        for step in C.STEPS:
            for sc in C.SCALARS:
                yield f'{path}-{step}-{sc}', C.step_case(path, step, sc, keep=(step == 9 and path != 'small'))
        for kind in C.SKIPS:
            for keep in (False, True):
                yield f'{path}-skip {kind}-keep{int(keep)}', C.skip_case(path, kind, keep)


def _shard_reports(variant=None):
    rep = C.Report()
    for shards, payload, found in C.shard_cases():
        flat, state = C.shard_pattern(shards, payload), C.make_state(found_inf=found)
        rep += C.poison_criteria(C.poison_shards(flat, shards, payload, state, variant), flat, shards, payload, state)
    for shards, payload, own, with_flat, rank in C.verdict_cases():
        flat, shard, state = C.verdict_flat(shards, payload, own, rank), C.own_shard(payload, own), C.make_state(found_inf=0.0, lr_mult=0.37)
        st, out = C.shard_verdict(shard, state, flat if with_flat else None, shards, payload, variant, rank)
        rep += C.verdict_criteria(st, out if with_flat else flat, shard, state, flat, shards, payload, with_flat)
    return rep


@functools.lru_cache(maxsize=None)
def _failures(variant, dtype=np.float32):
    """-> {criterion: [cases that fail it]} of one implementation (the twin, or the twin with one statement changed) over EVERY case"""
    failed = {}
    for name, case in _step_cases():
        got, state = C.run_model(case, dtype, variant)
        for crit in C.case_criteria(got, state, case).failed():
            failed.setdefault(crit, []).append(name)
    for row in C.COMMIT_TABLE:
        for crit in C.state_criteria(C.commit(row['state'], *row['rule'], row['flip'], variant), np.array(row['out'], F32)).failed():
            failed.setdefault(crit, []).append('commit: ' + row['name'])
    for r in _shard_reports(variant).failures():
        failed.setdefault(r[0], []).append('shards')
    return failed


def test_float32_twin_meets_every_criterion():
    """would catch a criterion that the arithmetic it describes cannot meet (a GPU failure would then say nothing): the float32 twin against the float64 definition's envelope and yardsticks on every path,
    step count, scalar set and skipped step, the exact models on the commit table and the shard layouts"""
    assert _failures(None) == {}
    case = C.step_case('ema', 9, 's65536_m.37_g3')
    rep = C.case_criteria(*C.run_model(case), case)
    print(f'\n{rep}')
    assert [r[0] for r in rep][:7] == ['gradient', 'm bits', 'v bits', 'p envelope', 'shadow envelope', 'shadow == half(p)', 'ema'] and len(rep) == 15


def test_yardstick_is_a_few_fp32_roundings():
    """would catch a bar that drifted wide: the twin's update against the definition's, relative to the operands' magnitude, over every case.
    Worked out, in ulp = 2^-23: the twelve roundings of the chain (inv_scale, g, the two products and the sum of m, v through the square
    root, the two divisions, + eps, lr lr_mult, step_size m) give at most 0.5 each, v's three give 1.75 behind the root: 7.25; the ONE rounding
    of pow(beta, t) passes through 1 - pow: at t = 2 half an ulp of 0.99^2 = 0.98 (2^-25) is 2^-25 / 0.0199 of bc2, half of that of its root:
    6.3, and 2^-25 / 0.19 = 1.3 in bc1.  Sum 14.9: the bar is 15 ulp (seen: 6.4), i.e. a yardstick under 7.2e-6 of the magnitude"""
    worst = max(C.twin_update_error(c['el'], c['state'], c['rule'], c['lr'], c['flags'])[0] for _, c in _step_cases())
    print(f'worst twin update error: {worst / 2.0 ** -23:.2f} ulp')
    assert 0 < worst <= 15 * 2.0 ** -23


# variant -> (a criterion that must reject it, a case that must be among the failing ones); the GPU test that applies the criterion to the
# kernels on that case is named in the comment
REJECTED_BY = {
    'eps inside the bias correction': ('p envelope', 'wide-0-s128'),                       # test_update_against_the_model[wide-0-*]
    'bc2 not square-rooted': ('p envelope', 'wide-9-s128'),                                # test_update_against_the_model[wide-9-*]
    'corrections from t': ('p envelope', 'wide-1-s128'),                                   # test_update_against_the_model[wide-1-*]
    'bias correction of m dropped': ('p envelope', 'wide-9-s3072_g3'),                     # the same
    'grad_mult dropped': ('m bits', 'wide-999-s3072_g3'),                                  # test_update_against_the_model[*-s3072_g3]
    'lr_mult dropped': ('p envelope', 'wide-29999-s3072_m.37'),                            # test_update_against_the_model[*-s3072_m.37]
    'unscale after squaring': ('v bits', 'wide-0-s128'),                                   # test_update_against_the_model
    'shadow from the old parameter': ('shadow envelope', 'wide-29999-s128'),               # the same
    'EMA on the parameter before the update': ('ema', 'ema-29999-s128'),                   # test_update_against_the_model[ema-*]
    'EMA not moved on a skipped step': ('ema', 'ema-skip found_inf-keep1'),                # test_skipped_step_against_the_model[ema-*]
    'step counted on a skipped step': ('state.step', 'commit: overflow'),                  # test_commit_table
    'found_inf not cleared': ('state.found_inf', 'commit: overflow'),                      # the same
    'growth at tracker + 1 > interval': ('state.scale', 'commit: tracker I-1'),            # the same
    'growth to inf applied': ('state.scale', 'commit: growth to inf withheld'),            # the same
    'parity flipped on a skipped step': ('state.parity', 'commit: skipped, parity 0, flip'),    # the same
    'dead cleared once the scale is finite again': ('state.dead', 'commit: dead is sticky'),    # the same
    'dead scale not an overflow in UPDATE': ('p unchanged', 'wide-skip scale 0-keep0'),    # test_skipped_step_against_the_model[*-scale 0-*]
    'poison only in shards with a gradient': ('poison buffer', 'shards'),                  # test_poison_shards
    'verdict cleans only its own shard': ('verdict flat', 'shards'),                       # test_shard_verdict
}


@pytest.mark.parametrize('variant', C.WRONG_VARIANTS)
def test_every_wrong_variant_is_rejected(variant):
    """each deliberately wrong model -- the twin with one statement changed, so that nothing but that statement can fail -- fails the criterion
    named in REJECTED_BY on the named case"""
    assert set(REJECTED_BY) == set(C.WRONG_VARIANTS)
    failed = _failures(variant)
    print(variant, '->', {k: len(v) for k, v in failed.items()})
    crit, case = REJECTED_BY[variant]
    assert crit in failed and case in failed[crit], failed.keys()


def test_wide_path_variants_fail_on_the_wide_path():
    """the argument of the pull request: every variant of the UPDATE arithmetic is rejected on a `wide` case, so a wide path with that arithmetic
    fails test_update_against_the_model[wide-...] (the EMA variants: the wide path has no EMA; they fail on `ema`)"""
    for variant in C.WRONG_VARIANTS[:8]:
        assert any(name.startswith('wide-') for names in _failures(variant).values() for name in names), variant


def test_trajectory_and_round_trip_models():
    """would catch a trajectory whose steps could be told apart by nothing (grow, back off, grow: the scale is another one in every step, the
    parity ends where it began after two flips) and a poison protocol that does not close in the models: one poisoning rank of two makes every
    shard's average NaN, and the verdict leaves the poisoned buffer finite"""
    state = C.make_state(**C.TRAJECTORY_STATE)
    r = C.TRAJECTORY_RULE
    scales = []
    for overflow in C.TRAJECTORY_OVERFLOW:
        if overflow:
            state[C.FOUND_INF] = 1.0
        state = C.commit(state, r['growth'], r['backoff'], r['interval'], 1)
        scales.append(float(state[C.SCALE]))
    assert scales == [6144.0, 3072.0, 6144.0] and state[C.STEP] == 10 and state[C.PARITY] == 0
    for shards, payload in ((2, 8), (65, 1000)):
        a = C.poison_shards(C.shard_pattern(shards, payload), shards, payload, C.make_state(found_inf=1.0))
        b = C.poison_shards(C.shard_pattern(shards, payload), shards, payload, C.make_state(found_inf=0.0))
        assert np.isnan(a[::payload]).all() and np.isnan(a).sum() == shards and C.same_bits(b, C.shard_pattern(shards, payload)) == 0
        avg = ((a.astype(F32) + b.astype(F32)) / 2).astype(F16)
        for rank in range(shards):
            st, _ = C.shard_verdict(avg[rank * payload:(rank + 1) * payload], C.make_state(), None, shards, payload)
            assert st[C.FOUND_INF] == 1
        _, cleaned = C.shard_verdict(avg[:payload], C.make_state(), a, shards, payload)
        assert np.isfinite(cleaned).all() and (cleaned[::payload] == 0).all()
