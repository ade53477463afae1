"""GPU: the optimizer kernels of csrc/optim.hip against the float64 model, cases and criteria of tests/optim_cases.py (whose header states
every bound's origin) -- each path of k_adam and k_adam_small_commit against the MODEL, not against another path; update_scale in both of its
kernels on the hand-written commit table; k_check_finite with one plant at a time; k_poison_shards and k_shard_verdict.  Called at the C ABI.
Outputs an entry must fill are NaN-filled first; every buffer sits between guard elements that must survive; buffers an entry must not touch
are compared bitwise with their input."""
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as C

pytestmark = pytest.mark.gpu

CHECK, UPDATE, COMMIT, FLIP = 1, 2, 4, 8
GUARD, SENTINEL = 8, 7.0          # elements in front of and behind every buffer (8 fp16 = 16 bytes: the aligned views stay 16-byte aligned)
F32, F16 = np.float32, np.float16
vp = ctypes.c_void_p


class Buffers:
    """named device buffers, each a view into a larger allocation filled with SENTINEL"""
    def __init__(self):
        self.big, self.view, self.start = {}, {}, {}

    def add(self, name, array, offset=False, nan=False):
        """offset: the view starts ONE element into the allocation (never 16-byte aligned); nan: NaN-filled instead of the array's values"""
        if array is None:
            self.view[name] = None
            return None
        t = torch.from_numpy(np.array(array, copy=True))
        start = 1 if offset else GUARD
        big = torch.full((t.numel() + 2 * GUARD,), SENTINEL, dtype=t.dtype, device='cuda')
        view = big[start:start + t.numel()]
        view.copy_(torch.full_like(t, float('nan')) if nan else t)
        assert (view.data_ptr() % 16 != 0) if offset else (view.data_ptr() % 16 == 0)
        self.big[name], self.view[name], self.start[name] = big, view, start
        return view

    def host(self, name):
        v = self.view[name]
        return None if v is None else v.cpu().numpy()

    def guards_intact(self):
        for name, big in self.big.items():
            n, s = self.view[name].numel(), self.start[name]
            if not (bool((big[:s] == SENTINEL).all()) and bool((big[s + n:] == SENTINEL).all())):
                return name
        return None


def _rule_args(rule):
    return [float(rule[k]) for k in ('beta1', 'beta2', 'eps', 'grad_mult', 'growth', 'backoff', 'interval')]


def _arrays(entries):
    """entries: dicts n, p, m, v, g, p16, is_half, lr (tensors or None) -> (count, the eight ctypes arrays as void*, the arrays kept alive)"""
    k = len(entries)
    if not k:
        return [0] + [None] * 8, []
    ptrs = lambda key: (vp * k)(*[None if e.get(key) is None else e[key].data_ptr() for e in entries])
    raw = [(ctypes.c_uint64 * k)(*[e['n'] for e in entries]), ptrs('p'), ptrs('m'), ptrs('v'), ptrs('g'), ptrs('p16'),
           (ctypes.c_int * k)(*[e['is_half'] for e in entries]), (ctypes.c_float * k)(*[float(e.get('lr', 0.0)) for e in entries])]
    return [k] + [ctypes.cast(a, vp) for a in raw], raw


def _step_ex(entries, rule, state, phases, omd=None):
    import _ngp_capi as capi
    args, keep = _arrays(entries)
    ema = (vp * len(entries))(*[e['ema'].data_ptr() for e in entries]) if omd is not None else None
    capi.check(capi.lib.ngp_optim_adam_step_ex(*args, *_rule_args(rule), state.data_ptr(), None if ema is None else ctypes.cast(ema, vp),
                                               0.0 if omd is None else float(omd), phases, capi.stream()))
    torch.cuda.synchronize()


def _small_commit(entries, rule, state, flip, table=None, table_grad=None, prefix=0):
    import _ngp_capi as capi
    args, keep = _arrays(entries)
    capi.check(capi.lib.ngp_optim_adam_small_commit(*args, *_rule_args(rule), state.data_ptr(), flip,
                                                    None if table is None else ctypes.cast(ctypes.pointer(table), vp),
                                                    None if table_grad is None else table_grad.data_ptr(), prefix, capi.stream()))
    torch.cuda.synchronize()


def _table(sets, state, rule, lr):
    """ngp_table_adam_t over two buffer sets (Buffers with p, m, v, p16)"""
    import _ngp_capi as capi
    ta = capi.TableAdam()
    for field, k in (('param', 'p'), ('exp_avg', 'm'), ('exp_avg_sq', 'v'), ('param_fp16', 'p16')):
        getattr(ta, field)[0], getattr(ta, field)[1] = sets[0].view[k].data_ptr(), sets[1].view[k].data_ptr()
    ta.state = state.data_ptr()
    ta.lr, ta.beta1, ta.beta2, ta.eps = float(lr), float(rule['beta1']), float(rule['beta2']), float(rule['eps'])
    return ta


def _state(words):
    t = torch.from_numpy(np.array(words, F32)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _entry(b, n, flags, lr, ema=False):
    return dict(n=n, p=b.view['p'], m=b.view['m'], v=b.view['v'], g=b.view['g'], p16=b.view['p16'], is_half=flags, lr=lr,
                ema=b.view['e'] if ema else None)


def _upload(el, offset=False, shadow_nan=False, nan=False, with_g=True):
    b = Buffers()
    for k in ('p', 'm', 'v'):
        b.add(k, el[k], offset, nan)
    b.add('p16', el['p16'], offset, nan or shadow_nan)
    b.add('g', el['g'] if with_g else None, offset)
    b.add('e', el.get('e'), offset)
    return b


def _got(b, g=None, ema=False):
    got = dict(p=b.host('p'), m=b.host('m'), v=b.host('v'), p16=b.host('p16'), g=b.host('g') if g is None else g)
    if ema:
        got['ema'] = b.host('e')
    return got


def _all_nan(b):
    return all(bool(torch.isnan(b.view[k].float()).all()) for k in ('p', 'm', 'v', 'p16'))


def _unchanged(b, el):
    return all(C.same_bits(b.host(k), np.asarray(el[k])) == 0 for k in ('p', 'm', 'v', 'p16') if el[k] is not None)


def _run(case):
    """one case on the GPU -> (got for the criteria, the state words afterwards); the buffers the launch must not touch are asserted here"""
    el, path, rule = case['el'], case['path'], case['rule']
    n = el['p'].size
    state = _state(case['state'])
    skip = C.adam_step(el, case['state'], rule, case['lr'], case['flags'])['skip']
    if path.startswith('prefix'):
        src = int(case['state'][C.PARITY] != 0)
        sets = [None, None]
        sets[src] = _upload(el, with_g=False)
        sets[src ^ 1] = _upload(el, nan=True, with_g=False)
        g = Buffers()
        g.add('g', el['g'])
        _small_commit([], rule, state, case['flip'], _table(sets, state, rule, case['lr']), g.view['g'], n)
        assert _unchanged(sets[src], el), 'the set the sweep reads was written'
        assert skip == _all_nan(sets[src ^ 1]), 'a skipped step wrote the other set' if skip else 'the other set was not filled'
        assert all(x.guards_intact() is None for x in (sets[0], sets[1], g))
        return _got(sets[src if skip else src ^ 1], g=g.host('g')), state.cpu().numpy()
    b = _upload(el, offset=case['offset'], shadow_nan=not skip)          # (a standing step must fill the whole shadow)
    entry = _entry(b, n, case['flags'], case['lr'], ema=case['omd'] is not None)
    if path == 'small':
        _small_commit([entry], rule, state, case['flip'])
    else:
        _step_ex([entry], rule, state, UPDATE, case['omd'])
    assert b.guards_intact() is None, b.guards_intact()
    return _got(b, ema=case['omd'] is not None), state.cpu().numpy()


def _judge(case, label):
    got, state = _run(case)
    rep = C.case_criteria(got, state, case)
    print(f'\n{label}\n{rep}')
    assert not rep.failures(), rep.failures()


@pytest.mark.parametrize('scalars', list(C.SCALARS))
@pytest.mark.parametrize('step', C.STEPS)
@pytest.mark.parametrize('path', list(C.PATHS))
def test_update_against_the_model(path, step, scalars):
    """would catch wrong Adam arithmetic in ANY one path (each is judged against the float64 model, so a shared error cannot hide): m and v
    that are not the fp32 twin's bits (unscale order, grad_mult, the order of (1 - beta2) g g), a parameter or shadow outside the powf envelope
    + yardstick (eps on the wrong side of the bias correction -- the v = 0 rows; bc2 not rooted; t instead of t + 1; lr_mult or bc1 dropped), a
    shadow that is not half(p_new), a gradient not zeroed or (step 9: keep bit) not kept, an EMA taken on the old parameter, a prefix sweep that
    reads the wrong set or writes the one it reads, and for the committing launches state words that are not update_scale's"""
    _judge(C.step_case(path, step, scalars, keep=(step == 9 and path != 'small')), f'{path} step {step} {scalars}')


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('kind', list(C.SKIPS))
@pytest.mark.parametrize('path', list(C.PATHS))
def test_skipped_step_against_the_model(path, kind, keep):
    """would catch a step that is not skipped as a whole: found_inf = 1 or 3, a scale of 0 or 2^-130 (1 / scale = inf: an overflow of its own)
    must leave p, m, v and the shadow bitwise unchanged, the gradient zeroed or (keep bit) unchanged, the other table set untouched (NaN), the
    EMA moved towards the UNCHANGED parameter; the committing launches back off, keep the step count and the parity, and raise `dead`"""
    _judge(C.skip_case(path, kind, keep), f'{path} skip {kind} keep {keep}')


def test_two_tensors_of_one_call_take_their_own_lr():
    """would catch a launch that applies tensor 0's learning rate (or length, or pointers) to tensor 1: the wide path (lr 1e-2) and the pair loop
    with its odd tail (lr 3e-4, one element into its allocation) in ONE ngp_optim_adam_step_ex call, each against the model"""
    cases = [C.step_case('wide', 9, 's65536_m.37_g3'), dict(C.step_case('pair', 9, 's65536_m.37_g3'), lr=C.LRS[1])]
    state = _state(cases[0]['state'])
    bufs = [_upload(c['el'], offset=c['offset'], shadow_nan=True) for c in cases]
    _step_ex([_entry(b, c['el']['p'].size, c['flags'], c['lr']) for b, c in zip(bufs, cases)], cases[0]['rule'], state, UPDATE)
    for b, c in zip(bufs, cases):
        rep = C.case_criteria(_got(b), state.cpu().numpy(), c)
        print(f'\nlr {c["lr"]}\n{rep}')
        assert not rep.failures() and b.guards_intact() is None


@pytest.mark.parametrize('entry', ['COMMIT', 'small_commit'])
@pytest.mark.parametrize('row', C.COMMIT_TABLE, ids=[r['name'] for r in C.COMMIT_TABLE])
def test_commit_table(row, entry):
    """would catch a loss-scale state machine that differs from the hand-written rows in either kernel that runs it (k_update_scale; the last
    workgroup of k_adam_small_commit, count = 0): growth at tracker + 1 >= interval and not before, growth to inf withheld with the tracker
    still reset, back-off into a denormal, 1 / scale = inf treated as an overflow and `dead` raised and kept, found_inf cleared, the step
    counted on standing steps only, the parity flipped only on a standing step with FLIP, lr_mult untouched, the ticket at 0"""
    growth, backoff, interval = row['rule']
    rule = C.make_rule(growth=growth, backoff=backoff, interval=interval)
    state = _state(row['state'])
    if entry == 'COMMIT':
        _step_ex([], rule, state, COMMIT | (FLIP if row['flip'] else 0))
    else:
        _small_commit([], rule, state, row['flip'])
    rep = C.state_criteria(state.cpu().numpy(), np.array(row['out'], F32))
    assert not rep.failures(), f'\n{rep}'


def test_three_step_trajectory_reads_the_words_the_last_commit_left():
    """would catch a step that takes t, the scale or found_inf from anywhere but the device words of the previous commit: CHECK | UPDATE |
    COMMIT three times with interval 1 (the scale doubles, halves on the planted inf of step 2, doubles again), each step judged against the
    model evaluated from what the device held before it"""
    r = C.TRAJECTORY_RULE
    rule = C.make_rule(r['grad_mult'], r['growth'], r['backoff'], r['interval'])
    el = C.path_elements('wide')
    b = _upload(el)
    state = _state(C.make_state(**C.TRAJECTORY_STATE))
    scales = []
    for overflow in C.TRAJECTORY_OVERFLOW:
        g = np.array(el['g'], copy=True)
        if overflow:
            g[C.N - 1] = np.inf
        b.view['g'].copy_(torch.from_numpy(g))
        b.view['p16'].fill_(float('nan') if not overflow else 0.5)
        before = dict(p=b.host('p'), m=b.host('m'), v=b.host('v'), p16=b.host('p16'), g=g)
        words = state.cpu().numpy()
        _step_ex([_entry(b, C.N, 1, C.LRS[0])], rule, state, CHECK | UPDATE | COMMIT)
        checked = C.check_finite([g], words)
        rep = C.step_criteria(_got(b), before, checked, rule, C.LRS[0], 1)
        rep = C.Report(rep + C.state_criteria(state.cpu().numpy(), C.commit(checked, rule['growth'], rule['backoff'], rule['interval'], 0)))
        print(f'\noverflow {overflow}\n{rep}')
        assert not rep.failures() and b.guards_intact() is None
        assert ('p unchanged' in [x[0] for x in rep]) == overflow
        scales.append(float(state[C.SCALE]))
    assert scales == [6144.0, 3072.0, 6144.0] and float(state[C.STEP]) == 10.0


def test_ticket_at_the_largest_grid():
    """would catch a ticket that commits early, twice or not at all when 224 workgroups draw it (192 prefix + 32 small-tensor workgroups, the
    launch's caps): three launches in a row -- standing, overflow, standing -- must each leave the commit model's words with the ticket back at
    0, flip the parity on the standing steps only, and every prefix and small-tensor element must match the model (a workgroup that read the
    state AFTER the commit would apply the next step's t, scale or parity)"""
    r = C.TRAJECTORY_RULE
    rule = C.make_rule(r['grad_mult'], r['growth'], r['backoff'], r['interval'])
    pre, small = C.ticket_elements()
    sets = [_upload(pre, with_g=False), _upload(pre, nan=True, with_g=False)]
    tg = Buffers()
    tg.add('g', pre['g'])
    sb = _upload(small)
    state = _state(C.make_state(**C.TRAJECTORY_STATE))
    table = _table(sets, state, rule, C.LRS[1])
    for overflow in C.TRAJECTORY_OVERFLOW:
        sb.view['g'].copy_(torch.from_numpy(small['g']))
        if overflow:
            state[C.FOUND_INF] = 1.0           # (as the gradient's producers raise it)
        words = state.cpu().numpy()
        src = int(words[C.PARITY] != 0)
        before = dict(p=sets[src].host('p'), m=sets[src].host('m'), v=sets[src].host('v'), p16=sets[src].host('p16'), g=pre['g'])
        other = {k: sets[src ^ 1].host(k) for k in ('p', 'm', 'v', 'p16')}
        before_small = dict(p=sb.host('p'), m=sb.host('m'), v=sb.host('v'), p16=sb.host('p16'), g=small['g'])
        _small_commit([_entry(sb, C.TICKET_SMALL, 1, C.LRS[0])], rule, state, 1, table, tg.view['g'], C.TICKET_PREFIX)
        after = state.cpu().numpy()
        rep = C.state_criteria(after, C.commit(words, rule['growth'], rule['backoff'], rule['interval'], 1))
        rep += C.step_criteria(_got(sets[src] if overflow else sets[src ^ 1], g=tg.host('g')), before, words, rule, C.LRS[1], 3)
        rep += C.step_criteria(_got(sb), before_small, words, rule, C.LRS[0], 1)
        print(f'\noverflow {overflow}\n{C.Report(rep)}')
        assert not C.Report(rep).failures()
        assert _unchanged(sets[src], before), 'the set the sweep reads was written'
        if overflow:
            assert all(C.same_bits(sets[src ^ 1].host(k), other[k]) == 0 for k in other), 'a skipped step wrote the other set'
        assert all(x.guards_intact() is None for x in (sets[0], sets[1], tg, sb))
    assert state.cpu().numpy().tolist()[:4] == [6144.0, 0.0, 0.0, 10.0] and float(state[C.PARITY]) == 0.0 and float(state[C.TICKET]) == 0.0


def test_check_finite_finds_one_plant_anywhere():
    """would catch a CHECK that misses a position: one inf, -inf or NaN at a time in the first element, the last element of the 8-wide body, the
    first and last element of the scalar tail, the one-element tail, a tail-only tensor, the fp32 branch's second grid-stride trip and last
    element, and the middle of each of the eight tensor slots; the unplanted call (65504, -65504, FLT_MAX, subnormals) must leave the word at 0,
    a word already raised must stay raised; every other state word and every gradient must be left as it was.  The fp16 tensors are slices of
    one flat buffer at offsets that are multiples of 8 elements, as optim.py lays its flat gradient buffer out"""
    tensors = C.check_tensors()
    offsets, total = [], 0
    for t in tensors:
        if t.dtype == F16:
            offsets.append(total)
            total += (t.size + 7) // 8 * 8
    flat_host = np.full(total, 3.0, F16)
    for t, off in zip([t for t in tensors if t.dtype == F16], offsets):
        flat_host[off:off + t.size] = t
    flat = Buffers()
    flat.add('flat', flat_host)
    f32 = Buffers()
    views, it = [], iter(offsets)
    for k, t in enumerate(tensors):
        if t.dtype == F16:
            off = next(it)
            views.append(flat.view['flat'][off:off + t.size])
        else:
            views.append(f32.add(f't{k}', t))
        assert views[-1].data_ptr() % 16 == 0
    entries = [dict(n=t.size, g=v, is_half=int(t.dtype == F16)) for t, v in zip(tensors, views)]
    rule = C.make_rule()

    def run(words):
        state = _state(words)
        _step_ex(entries, rule, state, CHECK)
        return state.cpu().numpy()

    clean = C.make_state(scale=3072.0, tracker=5.0, step=9.0, lr_mult=0.37, parity=1.0)
    assert not C.state_criteria(run(clean), C.check_finite(tensors, clean)).failures() and C.check_finite(tensors, clean)[C.FOUND_INF] == 0
    raised = C.make_state(found_inf=1.0)
    assert not C.state_criteria(run(raised), raised).failures()
    for name, k, e, val in C.check_plants():
        keep = views[k][e].clone()
        views[k][e] = val
        planted = [t.copy() for t in tensors]
        planted[k][e] = val
        got, want = run(clean), C.check_finite(planted, clean)
        views[k][e] = keep
        assert want[C.FOUND_INF] == 1 and not C.state_criteria(got, want).failures(), (name, k, e, val, got)
    assert C.same_bits(flat.host('flat'), flat_host) == 0 and all(C.same_bits(f32.host(f't{k}'), t) == 0 for k, t in enumerate(tensors) if t.dtype == F32)
    assert flat.guards_intact() is None and f32.guards_intact() is None


def _poison(flat, shards, payload, state):
    import _ngp_capi as capi
    capi.check(capi.lib.ngp_optim_poison_shards(flat.data_ptr(), shards, payload, state.data_ptr(), capi.stream()))
    torch.cuda.synchronize()


def _verdict(shard, state, flat, shards, payload):
    import _ngp_capi as capi
    capi.check(capi.lib.ngp_optim_shard_verdict(shard.data_ptr(), state.data_ptr(), None if flat is None else flat.data_ptr(), shards, payload, capi.stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize('shards,payload,found_inf', C.shard_cases())
def test_poison_shards(shards, payload, found_inf):
    """would catch a poison that misses a shard (the 65th: the launch has 64 lanes), lands off element r * payload, is written on a clean step,
    depends on what the shard holds (shard 1 is all zeros), or touches the state: the whole flat buffer, pre-filled with a pattern, bit for bit"""
    host, words = C.shard_pattern(shards, payload), C.make_state(found_inf=found_inf, lr_mult=0.37)
    b = Buffers()
    b.add('flat', host)
    state = _state(words)
    _poison(b.view['flat'], shards, payload, state)
    rep = C.poison_criteria(b.host('flat'), host, shards, payload, words) + C.state_criteria(state.cpu().numpy(), words)
    assert not C.Report(rep).failures() and b.guards_intact() is None, f'\n{C.Report(rep)}'
    assert int(np.isnan(b.host('flat')).sum()) == (shards if found_inf else 0)


@pytest.mark.parametrize('payload', C.PAYLOADS)
@pytest.mark.parametrize('shards', C.SHARDS)
def test_shard_verdict(shards, payload):
    """would catch a verdict that misses a non-finite class in element 0 of the own shard (NaN, +inf, -inf) or raises on a finite one, touches
    another state word, cleans only part of the flat buffer's shard heads (own shard only; not the 65th; not -inf), clears a finite head, or
    touches the flat buffer when it is not given"""
    for s, p, own, with_flat, rank in C.verdict_cases():
        if (s, p) != (shards, payload):
            continue
        host, shard_host, words = C.verdict_flat(shards, payload, own, rank), C.own_shard(payload, own), C.make_state(lr_mult=0.37, parity=1.0)
        b = Buffers()
        b.add('flat', host)
        b.add('shard', shard_host)
        state = _state(words)
        _verdict(b.view['shard'], state, b.view['flat'] if with_flat else None, shards, payload)
        rep = C.verdict_criteria(state.cpu().numpy(), b.host('flat'), shard_host, words, host, shards, payload, with_flat)
        assert not rep.failures() and b.guards_intact() is None, f'\nown {own} flat {with_flat} rank {rank}\n{rep}'
        assert C.same_bits(b.host('shard'), shard_host) == 0


@pytest.mark.parametrize('shards,payload', [(2, 8), (65, 1000)])
def test_poison_round_trip(shards, payload):
    """would catch a verdict protocol that does not close: rank A (found_inf raised) poisons, rank B does not; the buffers are averaged in torch as
    the reduce-scatter would; the verdict on EVERY shard of the average raises found_inf, and the verdict with A's flat buffer leaves it finite
    everywhere with +0 at the shard heads, the rest of the pattern intact"""
    host = C.shard_pattern(shards, payload)
    a, b = Buffers(), Buffers()
    a.add('flat', host)
    b.add('flat', host)
    _poison(a.view['flat'], shards, payload, _state(C.make_state(found_inf=1.0)))
    _poison(b.view['flat'], shards, payload, _state(C.make_state(found_inf=0.0)))
    avg = ((a.view['flat'].float() + b.view['flat'].float()) / 2).half()
    for rank in range(shards):
        state = _state(C.make_state())
        own = avg[rank * payload:(rank + 1) * payload].clone()
        _verdict(own, state, a.view['flat'] if rank == shards - 1 else None, shards, payload)
        assert state.cpu().numpy().tolist() == C.make_state(found_inf=1.0).tolist(), rank
    want = host.copy()
    want[::payload] = 0.0
    assert C.same_bits(a.host('flat'), want) == 0 and C.same_bits(b.host('flat'), host) == 0
    assert a.guards_intact() is None and b.guards_intact() is None
