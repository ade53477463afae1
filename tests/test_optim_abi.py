"""CPU checks of the optimizer entries' argument validation (csrc/optim.hip): every refusal happens before any device work, with the return
code and the message text pinned here word for word -- the texts the library printed before the entries came to share one marshalling
routine (`fill_opt_tensors`) and one state-pointer check, so that a restated check cannot drift.  No GPU: the device pointers are made up."""
import ctypes

import pytest

INVALID = 1
DEV = 4096               # a made-up device address, 16-byte aligned; no call below gets as far as a launch
RULE = (0.9, 0.99, 1e-15, 1.0, 2.0, 0.5, 2000.0)   # beta1, beta2, eps, grad_mult, growth, backoff, growth_interval
CHECK, UPDATE, COMMIT, FLIP = 1, 2, 4, 8


def _vp(a):
    return None if a is None else ctypes.cast(a, ctypes.c_void_p)


def _arrays(k, numel=64, **replace):
    """the eight per-tensor arrays of the Adam entries (n, params, exp_avg, exp_avg_sq, grads, params_fp16, grad_is_half, lr) for k tensors
    and the EMA array; replace: name -> None (a NULL array) or (index, None) (one NULL tensor)"""
    ptrs = lambda: (ctypes.c_void_p * max(k, 1))(*[DEV] * k)
    a = dict(n=(ctypes.c_uint64 * max(k, 1))(*[numel] * k), params=ptrs(), exp_avg=ptrs(), exp_avg_sq=ptrs(), grads=ptrs(), params_fp16=ptrs(),
             grad_is_half=(ctypes.c_int * max(k, 1))(*[1] * k), lr=(ctypes.c_float * max(k, 1))(*[1e-2] * k), ema=ptrs())
    for name, what in replace.items():
        if what is None:
            a[name] = None
        else:
            a[name][what[0]] = what[1]
    return a


def _step(lib, k, phases, state=DEV, ema=False, omd=0.0, **replace):
    a = _arrays(k, **replace)
    rc = lib.ngp_optim_adam_step_ex(k, _vp(a['n']), _vp(a['params']), _vp(a['exp_avg']), _vp(a['exp_avg_sq']), _vp(a['grads']), _vp(a['params_fp16']),
                                    _vp(a['grad_is_half']), _vp(a['lr']), *RULE, state, _vp(a['ema']) if ema else None, omd, phases, None)
    return rc, lib.ngp_last_error().decode()


def _table(capi, state=DEV, **replace):
    ta = capi.TableAdam()
    for f in ('param', 'exp_avg', 'exp_avg_sq', 'param_fp16'):
        getattr(ta, f)[0], getattr(ta, f)[1] = DEV, DEV
    ta.state = state
    ta.lr, ta.beta1, ta.beta2, ta.eps = 1e-2, 0.9, 0.99, 1e-15
    for f, k in replace.items():
        getattr(ta, f)[k] = None
    return ta


def _small(lib, k, state=DEV, table=None, tgrad=None, prefix=0, numel=64, **replace):
    a = _arrays(k, numel=numel, **replace)
    rc = lib.ngp_optim_adam_small_commit(k, _vp(a['n']), _vp(a['params']), _vp(a['exp_avg']), _vp(a['exp_avg_sq']), _vp(a['grads']), _vp(a['params_fp16']),
                                         _vp(a['grad_is_half']), _vp(a['lr']), *RULE, state, 1,
                                         None if table is None else ctypes.cast(ctypes.pointer(table), ctypes.c_void_p), tgrad, prefix, None)
    return rc, lib.ngp_last_error().decode()


def _ema(lib, k, **replace):
    a = _arrays(k, **replace)
    rc = lib.ngp_optim_ema_update(k, _vp(a['n']), _vp(a['params']), _vp(a['ema']), 0.01, None)
    return rc, lib.ngp_last_error().decode()


@pytest.fixture(scope='module')
def capi():
    import _ngp_capi
    return _ngp_capi


def test_state_pointer(capi):
    lib = capi.lib
    assert _step(lib, 1, CHECK | UPDATE | COMMIT, state=None) == (INVALID, 'optim_adam_step: NULL state')
    assert _step(lib, 1, CHECK | UPDATE | COMMIT, state=DEV + 8) == (INVALID, 'optim_adam_step: state (8 floats) must be 16-byte aligned')
    assert _small(lib, 1, state=None) == (INVALID, 'optim_adam_small_commit: NULL state')
    assert _small(lib, 1, state=DEV + 4) == (INVALID, 'optim_adam_small_commit: state (8 floats) must be 16-byte aligned')


def test_tensor_count(capi):
    lib = capi.lib
    assert _step(lib, 0, UPDATE) == (INVALID, 'optim_adam_step: between 1 and 8 tensors per call (got 0)')
    assert _step(lib, 9, CHECK) == (INVALID, 'optim_adam_step: between 1 and 8 tensors per call (got 9)')
    assert _small(lib, 9) == (INVALID, 'optim_adam_small_commit: at most 8 tensors per call (got 9)')
    assert _ema(lib, 0) == (INVALID, 'optim_ema_update: between 1 and 8 tensors per call (got 0)')


def test_phases(capi):
    lib = capi.lib
    subset = 'optim_adam_step: phases must be a non-empty subset of CHECK|UPDATE|COMMIT (+FLIP)'
    assert _step(lib, 1, 0) == (INVALID, subset)
    assert _step(lib, 1, FLIP) == (INVALID, subset)           # FLIP alone: none of the three phases
    assert _step(lib, 1, UPDATE | 16) == (INVALID, subset)    # an unknown bit
    assert _step(lib, 1, UPDATE | FLIP) == (INVALID, 'optim_adam_step: FLIP rides in the COMMIT phase')


@pytest.mark.parametrize('name', ['n', 'grads', 'grad_is_half', 'params', 'exp_avg', 'exp_avg_sq', 'lr'])
def test_null_array(capi, name):
    lib = capi.lib
    assert _step(lib, 2, UPDATE, **{name: None}) == (INVALID, 'optim_adam_step: NULL argument')
    assert _small(lib, 2, **{name: None}) == (INVALID, 'optim_adam_small_commit: NULL argument')
    if name in ('n', 'params'):
        assert _ema(lib, 2, **{name: None}) == (INVALID, 'optim_ema_update: NULL argument')
    if name in ('params', 'exp_avg', 'exp_avg_sq', 'lr'):
        # a CHECK-only call needs the gradients alone: with these arrays missing it gets past the array check (and stops at the NULL
        # gradient tensor planted here, still before any device work)
        assert _step(lib, 2, CHECK, grads=(0, None), **{name: None}) == (INVALID, 'optim_adam_step: NULL tensor 0')


def test_null_ema_array(capi):
    assert _ema(capi.lib, 2, ema=None) == (INVALID, 'optim_ema_update: NULL argument')


@pytest.mark.parametrize('count', [1, 3, 8])
@pytest.mark.parametrize('name', ['grads', 'params', 'exp_avg', 'exp_avg_sq'])
def test_null_tensor(capi, name, count):
    lib = capi.lib
    for k in sorted({0, count - 1}):
        assert _step(lib, count, UPDATE | COMMIT, **{name: (k, None)}) == (INVALID, f'optim_adam_step: NULL tensor {k}')
        assert _small(lib, count, **{name: (k, None)}) == (INVALID, f'optim_adam_small_commit: NULL tensor {k}')
        if name == 'params':
            assert _ema(lib, count, params=(k, None)) == (INVALID, f'optim_ema_update: NULL tensor {k}')
            assert _ema(lib, count, ema=(k, None)) == (INVALID, f'optim_ema_update: NULL tensor {k}')


def test_ema_decay_without_shadows(capi):
    lib = capi.lib
    assert _step(lib, 1, UPDATE, ema=False, omd=0.01) == (INVALID, 'optim_adam_step: EMA decay given without shadow tensors')
    # the array check comes first, the per-tensor check after it
    assert _step(lib, 1, UPDATE, ema=False, omd=0.01, lr=None) == (INVALID, 'optim_adam_step: NULL argument')
    assert _step(lib, 1, UPDATE, ema=False, omd=0.01, grads=(0, None)) == (INVALID, 'optim_adam_step: EMA decay given without shadow tensors')


def test_table_prefix(capi):
    lib = capi.lib
    needs = ('optim_adam_small_commit: a table prefix needs the table\'s buffer sets (on the same state) and its stored fp16 gradient')
    assert _small(lib, 1, table=None, tgrad=DEV, prefix=64) == (INVALID, needs)
    assert _small(lib, 1, table=_table(capi), tgrad=None, prefix=64) == (INVALID, needs)
    assert _small(lib, 1, table=_table(capi, state=DEV + 32), tgrad=DEV, prefix=64) == (INVALID, needs)
    for prefix in (2, 63, 65):
        assert _small(lib, 0, table=_table(capi), tgrad=DEV, prefix=prefix) == \
            (INVALID, 'optim_adam_small_commit: table_prefix_params must be a multiple of 4')
    for field in ('param', 'exp_avg', 'exp_avg_sq', 'param_fp16'):
        for k in (0, 1):
            assert _small(lib, 1, table=_table(capi, **{field: k}), tgrad=DEV, prefix=64) == \
                (INVALID, f'optim_adam_small_commit: NULL buffer in table set {k}')
    # both sets incomplete: the first one is named
    assert _small(lib, 1, table=_table(capi, param=1, exp_avg=0), tgrad=DEV, prefix=64)[1] == 'optim_adam_small_commit: NULL buffer in table set 0'


def test_small_commit_cap(capi):
    lib = capi.lib
    cap = 1 << 22
    text = 'optim_adam_small_commit: %d parameters -- this entry serves small tensors (<= 4 M); use ngp_optim_adam_step_ex'
    assert _small(lib, 1, numel=cap + 1) == (INVALID, text % (cap + 1))
    assert _small(lib, 2, numel=cap // 2 + 1) == (INVALID, text % (cap + 2))
    assert _small(lib, 1, numel=cap - 60, table=_table(capi), tgrad=DEV, prefix=64) == (INVALID, text % (cap + 4))   # the prefix counts


def test_ema_update(capi):
    lib = capi.lib
    assert _ema(lib, 9) == (INVALID, 'optim_ema_update: between 1 and 8 tensors per call (got 9)')
    assert _ema(lib, 1, params=(0, None)) == (INVALID, 'optim_ema_update: NULL tensor 0')
