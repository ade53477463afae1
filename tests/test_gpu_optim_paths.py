"""GPU: one seeded element set through every path of csrc/optim.hip that claims the same arithmetic -- k_adam's wide path, its pair loop with the
odd tail, its general path on an fp32 gradient, and the small-tensor loop and the table-prefix sweep of k_adam_small_commit.  The resulting
parameters, moments and fp16 shadows must be bitwise equal element for element; a skipped step must leave them bitwise unchanged; the commit
inside ngp_optim_adam_small_commit must leave the state words that UPDATE|COMMIT of ngp_optim_adam_step_ex leaves.  Called at the C ABI."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4104                 # 1026 four-element groups over the launch's 3 workgroups x 256 lanes: two grid-stride trips of the wide loop
LR, BETA1, BETA2, EPS = 1e-2, 0.9, 0.99, 1e-15
RULE = (BETA1, BETA2, EPS, 1.0, 2.0, 0.5, 2000.0)   # ..., grad_mult, growth, backoff, growth_interval
SCALE, STEP, LR_MULT = 128.0, 3.0, 0.5
UPDATE, COMMIT = 2, 4


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.half else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(found_inf=0.0):
    return torch.tensor([SCALE, 0.0, found_inf, STEP, LR_MULT, 0.0, 0.0, 0.0], device='cuda')


@pytest.fixture(scope='module')
def data():
    gen = torch.Generator().manual_seed(20)
    p = torch.randn(N, generator=gen) * 1e-2
    m = torch.randn(N, generator=gen) * 1e-3
    v = (torch.randn(N, generator=gen) * 1e-3) ** 2
    g = (torch.randn(N, generator=gen) * 4.0).half()                         # ordinary loss-scaled values
    g[torch.arange(1, N, 7)] = 0.0                                             # exact zeros
    sub = torch.arange(3, N, 11)
    g[sub] = (torch.arange(sub.numel()) % 1023 + 1).float().mul(2.0 ** -24).half() * (1 - 2 * (torch.arange(sub.numel()) % 2)).half()   # subnormals
    big = torch.arange(5, N, 13)
    g[big] = torch.tensor([65504.0, -65504.0, 65472.0, -65472.0, 65024.0, -64512.0]).half().repeat(big.numel() // 6 + 1)[:big.numel()]
    assert torch.isfinite(g.float()).all() and (g == 0).sum() > 400 and ((g != 0) & (g.abs() < 6e-5)).sum() > 300 and (g.abs() > 64000).sum() > 300
    assert g[N - 2] != 0 and g[N - 2].abs() < 100   # the odd tail of the 4103-element run carries an ordinary value
    return {k: t.cuda() for k, t in dict(p=p, m=m, v=v, g=g).items()}


def _offset_view(t, n):
    """elements [0, n) of t in a view that starts one element into a larger allocation (never 16-byte aligned)"""
    big = torch.zeros(t.numel() + 8, dtype=t.dtype, device='cuda')
    big[1:1 + n].copy_(t[:n])
    return big[1:1 + n]


def _tensors(data, n=N, offset=False, g32=False, shadow=True):
    mk = (lambda t: _offset_view(t, n)) if offset else (lambda t: t[:n].clone())
    t = dict(p=mk(data['p']), m=mk(data['m']), v=mk(data['v']), g=mk(data['g'].float() if g32 else data['g']))
    t['p16'] = mk(data['p'].half()) if shadow else None
    if offset:
        assert all(x.data_ptr() % 16 != 0 for x in (t['p'], t['m'], t['v']))
    else:
        assert all(x.data_ptr() % 16 == 0 for x in t.values() if x is not None)
    return t


_KEEP = []


def _arrays(t, n, is_half):
    vp = ctypes.c_void_p
    one = lambda x: (vp * 1)(None if x is None else x.data_ptr())
    raw = [(ctypes.c_uint64 * 1)(n), one(t['p']), one(t['m']), one(t['v']), one(t['g']), one(t['p16']), (ctypes.c_int * 1)(is_half), (ctypes.c_float * 1)(LR)]
    _KEEP[:] = raw   # (alive until the next call: every caller synchronises before it returns)
    return [1] + [ctypes.cast(a, vp) for a in raw]


def _step(t, state, n=N, is_half=1, phases=UPDATE):
    import _ngp_capi as capi
    capi.check(capi.lib.ngp_optim_adam_step_ex(*_arrays(t, n, is_half), *RULE, state.data_ptr(), None, 0.0, phases, capi.stream()))
    torch.cuda.synchronize()
    return t


def _small(t, state, is_half=1, flip=0):
    import _ngp_capi as capi
    capi.check(capi.lib.ngp_optim_adam_small_commit(*_arrays(t, N, is_half), *RULE, state.data_ptr(), flip, None, None, 0, capi.stream()))
    torch.cuda.synchronize()
    return t


def _prefix(data, state, flip=1):
    """the data as the table prefix: buffer set 0 holds it (parity 0), set 1 is NaN-filled; returns (set 0, set 1, the stored gradient)"""
    import _ngp_capi as capi
    s0 = _tensors(data)
    s1 = {k: torch.full_like(s0[k], float('nan')) for k in ('p', 'm', 'v', 'p16')}
    ta = capi.TableAdam()
    for field, k in (('param', 'p'), ('exp_avg', 'm'), ('exp_avg_sq', 'v'), ('param_fp16', 'p16')):
        getattr(ta, field)[0], getattr(ta, field)[1] = s0[k].data_ptr(), s1[k].data_ptr()
    ta.state = state.data_ptr()
    ta.lr, ta.beta1, ta.beta2, ta.eps = LR, BETA1, BETA2, EPS
    capi.check(capi.lib.ngp_optim_adam_small_commit(0, None, None, None, None, None, None, None, None, *RULE, state.data_ptr(), flip,
                                                    ctypes.cast(ctypes.pointer(ta), ctypes.c_void_p), s0['g'].data_ptr(), N, capi.stream()))
    torch.cuda.synchronize()
    return s0, s1, s0['g']


@pytest.fixture(scope='module')
def wide(data):
    """path 1: fp16 gradient + shadow on aligned buffers -- the reference of every comparison below (never written after this)"""
    t = _step(_tensors(data), _state())
    assert not _same(t['p'], data['p']) and not _same(t['m'], data['m']) and not _same(t['v'], data['v'])   # the step stood
    assert all(torch.isfinite(t[k].float()).all() for k in ('p', 'm', 'v', 'p16'))
    assert _same(t['p16'], t['p'].half()) and not t['g'].any()          # the shadow of the updated weights; the gradient zeroed
    return t


def test_pair_loop_and_odd_tail_equal_the_wide_path(data, wide):
    t = _step(_tensors(data, n=N - 1, offset=True), _state(), n=N - 1)
    for k in ('p', 'm', 'v', 'p16'):
        assert _same(t[k], wide[k][:N - 1]), k
    assert not t['g'].any()


def test_fp32_gradient_equals_the_wide_path(data, wide):
    t = _step(_tensors(data, g32=True, shadow=False), _state(), is_half=0)
    for k in ('p', 'm', 'v'):
        assert _same(t[k], wide[k]), k
    assert not t['g'].any()


def test_small_tensor_loop_equals_the_wide_path_and_commits_like_update_commit(data, wide):
    state = _state()
    t = _small(_tensors(data), state, flip=0)
    for k in ('p', 'm', 'v', 'p16'):
        assert _same(t[k], wide[k]), k
    assert not t['g'].any()
    ref = _state()
    _step(_tensors(data), ref, phases=UPDATE | COMMIT)
    assert _same(state, ref), (state, ref)
    assert state.tolist() == [SCALE, 1.0, 0.0, STEP + 1.0, LR_MULT, 0.0, 0.0, 0.0]


def test_table_prefix_sweep_equals_the_wide_path_and_flips(data, wide):
    state = _state()
    s0, s1, g = _prefix(data, state, flip=1)
    for k in ('p', 'm', 'v', 'p16'):
        assert _same(s1[k], wide[k]), k
    assert _same(s0['p'], data['p']) and _same(s0['m'], data['m']) and _same(s0['v'], data['v']) and _same(s0['p16'], data['p'].half())
    assert _same(g, data['g'])                                            # the stored table gradient is read, never written
    assert state.tolist() == [SCALE, 1.0, 0.0, STEP + 1.0, LR_MULT, 1.0, 0.0, 0.0]   # parity flipped, ticket back at 0


@pytest.mark.parametrize('keep', [False, True])
def test_skipped_step_changes_nothing(data, keep):
    is_half = 3 if keep else 1

    def unchanged(t, n=N):
        for k, want in (('p', data['p']), ('m', data['m']), ('v', data['v']), ('p16', data['p'].half())):
            assert _same(t[k], want[:n]), k
        assert _same(t['g'], data['g'][:n]) if keep else not t['g'].any()

    unchanged(_step(_tensors(data), _state(1.0), is_half=is_half))
    unchanged(_step(_tensors(data, n=N - 1, offset=True), _state(1.0), n=N - 1, is_half=is_half), N - 1)
    state = _state(1.0)
    unchanged(_small(_tensors(data), state, is_half=is_half, flip=0))
    assert state.tolist() == [SCALE * 0.5, 0.0, 0.0, STEP, LR_MULT, 0.0, 0.0, 0.0]    # backed off, step count kept
    if not keep:   # (the prefix takes no keep bit: its gradient is the table's stored one)
        state = _state(1.0)
        s0, s1, g = _prefix(data, state, flip=1)
        assert all(torch.isnan(s1[k].float()).all() for k in ('p', 'm', 'v', 'p16'))
        assert _same(s0['p'], data['p']) and _same(s0['m'], data['m']) and _same(s0['v'], data['v']) and _same(g, data['g'])
        assert state.tolist() == [SCALE * 0.5, 0.0, 0.0, STEP, LR_MULT, 0.0, 0.0, 0.0]   # a skipped step does not flip
