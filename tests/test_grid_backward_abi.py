"""CPU checks of the grid backward's entries (csrc/gridencoder.hip): every refusal that happens before any device work, with the return code
and the message text pinned word for word, and the values of the two host-only queries (ngp_grid_backward_workspace_bytes,
ngp_grid_table_adam_prefix) pinned as literals -- the texts and numbers the library gave before the entry body was split into named steps and
the plan words got names, so that a restated check or plan rule cannot drift.  No GPU: the device pointers are made up."""
import ctypes

import numpy as np
import pytest

import oracle

OK, INVALID = 0, 1
DEV = 4096               # a made-up device address; no call below gets as far as a memset or a launch
F32, F16, F64 = 0, 1, 2
MIN_SAMPLES = 16384      # BIN_MIN_SAMPLES

LEGO = dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048)   # tests/test_gpu_grid.py
SMALL = dict(num_levels=8, level_dim=2, per_level_scale=1.9, base_resolution=8, log2_hashmap_size=15)
T1 = dict(input_dim=3, **SMALL)
T2 = dict(input_dim=2, **SMALL)
T3 = dict(input_dim=3, num_levels=4, level_dim=2, per_level_scale=1.5, base_resolution=64, log2_hashmap_size=20)
ADAM20 = dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=20, desired_resolution=2048)  # tests/test_gpu_table_adam.py


@pytest.fixture(scope='module')
def capi():
    import _ngp_capi
    return _ngp_capi


def _host(offs):
    return (ctypes.c_int32 * len(offs))(*[int(v) for v in offs])


def _table(cfg):
    offs, pls = oracle.grid_offsets(**cfg)
    return offs, float(np.log2(pls)), cfg['base_resolution'], cfg['input_dim'], cfg['num_levels']


def _call(capi, entry='slabs', B=MIN_SAMPLES, D=3, C=2, L=2, S=0.0, H=16, dtype=F16, bound=0.0, grad=DEV, inputs=DEV, offsets=DEV, ge=DEV, dy_dx=None,
          grad_inputs=None, gridtype=0, host=None, ws=None, ws_bytes=0, found_inf=None, sets=None):
    lib = capi.lib
    harr = None if host is None else _host(host)
    hp = None if harr is None else ctypes.cast(harr, ctypes.c_void_p)
    head = (grad, inputs, None, offsets, ge, B, D, C, L, S, H, dy_dx, grad_inputs, gridtype, 0, 0, dtype)
    if entry == 'plain':
        rc = lib.ngp_grid_encode_backward(*head, None)
    elif entry == 'ex':
        rc = lib.ngp_grid_encode_backward_ex(*head, bound, None)
    elif entry == 'ws':
        rc = lib.ngp_grid_encode_backward_ws(*head, bound, hp, ws, ws_bytes, None)
    elif entry == 'checked':
        rc = lib.ngp_grid_encode_backward_checked(*head, bound, hp, ws, ws_bytes, found_inf, None)
    else:
        rc = lib.ngp_grid_encode_backward_checked_slabs(*head, bound, hp, ws, ws_bytes, found_inf, None if sets is None else ctypes.byref(sets), None)
    return rc, lib.ngp_last_error().decode()


ENTRIES = ('plain', 'ex', 'ws', 'checked', 'slabs')


@pytest.mark.parametrize('entry', ENTRIES)
def test_shape_refusals(capi, entry):
    fn = 'grid_encode_backward'
    assert _call(capi, entry, D=1) == (INVALID, f'{fn}: GridEncoding: input dim D must be 2, 3, 4 or 5 (got 1)')
    assert _call(capi, entry, D=6) == (INVALID, f'{fn}: GridEncoding: input dim D must be 2, 3, 4 or 5 (got 6)')
    assert _call(capi, entry, C=3) == (INVALID, f'{fn}: GridEncoding: C must be 1, 2, 4, or 8. (got 3)')
    assert _call(capi, entry, L=0) == (INVALID, f'{fn}: number of levels must be in [1, 32] (got 0)')
    assert _call(capi, entry, L=33) == (INVALID, f'{fn}: number of levels must be in [1, 32] (got 33)')
    assert _call(capi, entry, dtype=7) == (INVALID, f'{fn}: embeddings must be float32 or float16')
    assert _call(capi, entry, D=1, C=3, L=0, dtype=7)[1] == f'{fn}: GridEncoding: input dim D must be 2, 3, 4 or 5 (got 1)'   # D first
    if entry in ('checked', 'slabs'):
        assert _call(capi, entry, dtype=F64) == (INVALID, f'{fn}: float64 is not provided by this entry point')


@pytest.mark.parametrize('entry', ENTRIES)
def test_null_tensors_and_the_empty_batch(capi, entry):
    for name in ('grad', 'inputs', 'offsets', 'ge'):
        assert _call(capi, entry, **{name: None}) == (INVALID, 'grid_encode_backward: NULL tensor')
        assert _call(capi, entry, B=0, **{name: None})[0] == OK          # an empty batch touches nothing
    assert _call(capi, entry, B=0, D=1)[0] == INVALID                     # ... but its shape is checked


@pytest.mark.parametrize('entry', ENTRIES[1:])
def test_bound_with_dy_dx(capi, entry):
    text = 'grid_encode_backward: the fused input mapping does not provide grad_inputs'
    assert _call(capi, entry, bound=1.0, dy_dx=DEV, grad_inputs=DEV) == (INVALID, text)
    assert _call(capi, entry, bound=1.0, dy_dx=DEV, D=1) == (INVALID, text)   # in front of the shape checks


@pytest.mark.parametrize('entry', ENTRIES[3:])
def test_found_inf_needs_host_offsets(capi, entry):
    text = 'grid_encode_backward: found_inf needs the host copy of the offsets'
    assert _call(capi, entry, found_inf=DEV) == (INVALID, text)
    assert _call(capi, entry, found_inf=DEV, C=3) == (INVALID, text)
    assert _call(capi, entry, found_inf=DEV, bound=1.0, dy_dx=DEV)[1] == 'grid_encode_backward: the fused input mapping does not provide grad_inputs'


def test_workspace_too_small(capi):
    offs, S, H, D, L = _table(T1)
    need = int(capi.lib.ngp_grid_backward_workspace_bytes(ctypes.cast(_host(offs), ctypes.c_void_p), MIN_SAMPLES, D, 2, L, S, H, 0, 0, F16))
    for entry in ('ws', 'checked', 'slabs'):
        assert _call(capi, entry, D=D, L=L, S=S, H=H, host=offs, ws=DEV, ws_bytes=need - 1) == \
            (INVALID, f'grid_encode_backward: workspace of {need - 1} bytes, ngp_grid_backward_workspace_bytes() asks for {need}')


def _sets(capi, **fields):
    s = capi.SlabSets()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def test_slab_set_refusals(capi):
    null = 'grid_encode_backward: NULL tensor in the slab sets'
    for x in 'ab':
        assert _call(capi, sets=_sets(capi, **{'n_slabs_' + x: 2, 'n_params_' + x: 64, 'grad_weights_' + x: DEV})) == (INVALID, null)   # slabs missing
        assert _call(capi, sets=_sets(capi, **{'slabs_' + x: DEV, 'n_slabs_' + x: 2, 'n_params_' + x: 64})) == (INVALID, null)          # output missing
        # a set without slabs is swept for found_inf only: its gradients must be there
        assert _call(capi, sets=_sets(capi, **{'n_params_' + x: 64}), found_inf=DEV, host=[0, 8, 16]) == (INVALID, null)
    assert _call(capi, sets=_sets(capi, slabs_a=DEV, n_slabs_a=2, n_params_a=64), D=1) == (INVALID, null)    # in front of every other check
    loss = 'grid_encode_backward: loss sum without per-ray errors'
    assert _call(capi, sets=_sets(capi, loss=DEV)) == (INVALID, loss)
    assert _call(capi, sets=_sets(capi, loss=DEV, ray_err=DEV, n_rays=0)) == (INVALID, loss)
    assert _call(capi, sets=_sets(capi, loss=DEV, n_rays=16)) == (INVALID, loss)
    assert _call(capi, sets=_sets(capi, loss=DEV, slabs_b=DEV, n_slabs_b=1, n_params_b=64)) == (INVALID, null)   # the sets first


def test_overwrite_of_an_empty_batch_needs_the_table(capi):
    text = 'grid_encode_backward: overwrite_table needs the table and the host copy of the offsets'
    assert _call(capi, B=0, sets=_sets(capi, overwrite_table=1)) == (INVALID, text)
    assert _call(capi, B=0, ge=None, host=[0, 8, 16], sets=_sets(capi, overwrite_table=1)) == (INVALID, text)


def _adam(capi, state=DEV, **null):
    ta = capi.TableAdam()
    for f in ('param', 'exp_avg', 'exp_avg_sq', 'param_fp16'):
        getattr(ta, f)[0], getattr(ta, f)[1] = DEV, DEV
    ta.state = state
    ta.lr, ta.beta1, ta.beta2, ta.eps = 1e-2, 0.9, 0.99, 1e-15
    for f, k in null.items():
        getattr(ta, f)[k] = None
    return ta


def _adam_call(capi, ta, overwrite=1, **kw):
    s = _sets(capi, overwrite_table=overwrite, table_adam=ctypes.cast(ctypes.pointer(ta), ctypes.c_void_p))
    return _call(capi, sets=s, **kw)


def test_table_adam_refusals(capi):
    needs = ('grid_encode_backward: table_adam needs overwrite_table and every level on the record-sort path (fp16, C = 2, >= 16384 samples, '
             'a workspace and the host offsets)')
    offs, S, H, D, L = _table(T1)
    good = dict(D=D, L=L, S=S, H=H, host=offs, ws=DEV, ws_bytes=1 << 30)
    assert _adam_call(capi, _adam(capi), B=0, **good) == (INVALID, 'grid_encode_backward: table_adam with an empty batch')
    assert _adam_call(capi, _adam(capi), overwrite=0, **good) == (INVALID, needs)
    assert _adam_call(capi, _adam(capi), **dict(good, B=MIN_SAMPLES - 1)) == (INVALID, needs)
    assert _adam_call(capi, _adam(capi), **dict(good, ws=None)) == (INVALID, needs)
    assert _adam_call(capi, _adam(capi), **dict(good, host=None)) == (INVALID, needs)
    assert _adam_call(capi, _adam(capi), **dict(good, dtype=F32)) == (INVALID, needs)
    assert _adam_call(capi, _adam(capi), **dict(good, C=4)) == (INVALID, needs)
    o3, S3, H3, D3, L3 = _table(T3)   # one atomic level
    assert _adam_call(capi, _adam(capi), D=D3, L=L3, S=S3, H=H3, host=o3, ws=DEV, ws_bytes=1 << 30) == (INVALID, needs)
    assert _adam_call(capi, _adam(capi, state=None), **good) == (INVALID, 'grid_encode_backward: table_adam without the optimizer\'s state')
    # the table gradient may be NULL with table_adam -- unless dense levels leave their entries to the closing launch
    assert _adam_call(capi, _adam(capi), **dict(good, ge=None)) == \
        (INVALID, 'grid_encode_backward: table_adam: the dense levels\' gradient needs grad_embeddings')
    for field in ('param', 'exp_avg', 'exp_avg_sq', 'param_fp16'):
        for k in (0, 1):
            assert _adam_call(capi, _adam(capi, **{field: k}), **good) == (INVALID, f'grid_encode_backward: table_adam: NULL buffer in set {k}')
    assert _adam_call(capi, _adam(capi, param=1, exp_avg=0), **good)[1] == 'grid_encode_backward: table_adam: NULL buffer in set 0'
    # two levels of one scale (S = 0, H = 16: 17^3 = 4913 vertices): 4096 entries are hashed, 4920 dense -- a dense level behind a hashed one
    behind = dict(D=3, L=2, S=0.0, H=16, ws=DEV, ws_bytes=1 << 30)
    assert _adam_call(capi, _adam(capi), host=[0, 4096, 4096 + 4920], **behind) == \
        (INVALID, 'grid_encode_backward: table_adam: a dense level behind a hashed one (level 1)')
    assert _adam_call(capi, _adam(capi), host=[0, 4920, 4920 + 4096, 2 * 4920 + 4096, 2 * 4920 + 2 * 4096], **dict(behind, L=4)) == \
        (INVALID, 'grid_encode_backward: table_adam: a dense level behind a hashed one (level 2)')
    assert _adam_call(capi, _adam(capi), inputs=None, ge=None, **good) == (INVALID, 'grid_encode_backward: NULL tensor')   # in front of the admission
    assert _adam_call(capi, _adam(capi), grad=None, **good) == (INVALID, 'grid_encode_backward: NULL tensor')


def test_fp64_branch_of_ws(capi):
    fn = 'grid_encode_backward'
    f64 = dict(entry='ws', dtype=F64)
    assert _call(capi, D=6, **f64) == (INVALID, f'{fn}: GridEncoding: input dim D must be 2, 3, 4 or 5 (got 6)')
    assert _call(capi, C=5, **f64) == (INVALID, f'{fn}: GridEncoding: C must be 1, 2, 4, or 8. (got 5)')
    assert _call(capi, L=40, **f64) == (INVALID, f'{fn}: number of levels must be in [1, 32] (got 40)')
    assert _call(capi, bound=1.0, **f64) == (INVALID, f'{fn}: float64 is not provided with the fused input mapping')
    assert _call(capi, bound=1.0, B=0, **f64) == (INVALID, f'{fn}: float64 is not provided with the fused input mapping')
    assert _call(capi, B=0, grad=None, **f64)[0] == OK
    for name in ('grad', 'inputs', 'offsets', 'ge'):
        assert _call(capi, **{name: None}, **f64) == (INVALID, f'{fn}: NULL tensor')
    both = f'{fn}: dy_dx and grad_inputs must both be given or both be NULL'
    assert _call(capi, dy_dx=DEV, **f64) == (INVALID, both)
    assert _call(capi, grad_inputs=DEV, **f64) == (INVALID, both)
    for entry in ('plain', 'ex'):   # these forward through _ws as well
        assert _call(capi, entry, dtype=F64, dy_dx=DEV) == (INVALID, both)


# ---------------------------------------------------------------------------------------------------------------------
# the host-only queries: literals read from the library before the plan words got names
# ---------------------------------------------------------------------------------------------------------------------
def _query(capi, which, cfg, B, C=2, dtype=F16, gridtype=0, align=0, D=None):
    offs, S, H, D0, L = _table(cfg)
    fn = getattr(capi.lib, which)
    return int(fn(ctypes.cast(_host(offs), ctypes.c_void_p), B, D0 if D is None else D, C, L, S, H, gridtype, align, dtype))


WORKSPACE = {
    ('LEGO', 16383): 0, ('LEGO', 16384): 17039424, ('LEGO', 16421): 17571904, ('LEGO', 49152): 51118144,
    ('T1', 16384): 8442944, ('T1', 16421): 8706880, ('T2', 16384): 4279360, ('T2', 16421): 4413248, ('T3', 16384): 3227712, ('T3', 16421): 3328576,
}
NONE = 0xffffffff
PREFIX = {
    ('LEGO', 16383): NONE, ('LEGO', 16384): 352696, ('LEGO', 16421): 352696, ('LEGO', 49152): 352696,
    ('T1', 16384): 32656, ('T1', 16421): 32656, ('T2', 16384): 15664, ('T2', 16421): 15664, ('T3', 16384): NONE, ('T3', 16421): NONE,   # T3: one atomic level
    ('ADAM20', 16384): NONE, ('ADAM20', 262144): NONE,
}
TABLES = dict(LEGO=LEGO, T1=T1, T2=T2, T3=T3, ADAM20=ADAM20)


@pytest.mark.parametrize('name,B', sorted(WORKSPACE))
def test_workspace_bytes(capi, name, B):
    assert _query(capi, 'ngp_grid_backward_workspace_bytes', TABLES[name], B) == WORKSPACE[(name, B)]


def test_workspace_bytes_of_shapes_off_the_record_sort_path(capi):
    for cfg in (LEGO, T1, T3):
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', cfg, 49152, dtype=F32) == 0
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', cfg, 49152, C=4) == 0
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', cfg, 49152, D=4) == 0
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', cfg, (1 << 24) + 1) == 0
    assert capi.lib.ngp_grid_backward_workspace_bytes(None, 49152, 3, 2, 16, 1.0, 16, 0, 0, F16) == 0


@pytest.mark.parametrize('name,B', sorted(PREFIX))
def test_table_adam_prefix(capi, name, B):
    assert _query(capi, 'ngp_grid_table_adam_prefix', TABLES[name], B) == PREFIX[(name, B)]


def test_table_adam_prefix_of_shapes_off_the_record_sort_path(capi):
    for kw in (dict(dtype=F32), dict(C=4), dict(D=4)):
        assert _query(capi, 'ngp_grid_table_adam_prefix', T1, 16384, **kw) == 0xffffffff
    assert capi.lib.ngp_grid_table_adam_prefix(None, 16384, 3, 2, 8, 1.0, 8, 0, 0, F16) == 0xffffffff


def test_plan_rule_of_the_three_small_tables(capi):
    """what the tests of tests/test_gpu_grid_backward_paths.py rely on, from the sizes alone (BIN_SLICE = 4096 entries, 128 round-robin bins for a
    dense level of at most 128 * 4096 entries, at most 512 bins): descriptors = sum over sorted levels of bins * chunks, records = 2^D * 512 per
    chunk and sorted level"""
    def expect(cfg, B, sorted_levels):
        offs, S, H, D, L = _table(cfg)
        chunks = -(-B // 512)
        sizes = np.diff(offs)
        desc = sum((128 if dense else -(-int(sizes[l]) // 4096)) * chunks for l, dense in sorted_levels)
        return ((desc * 4 + 255) & ~255) + len(sorted_levels) * chunks * 512 * (1 << D) * 8 + 64
    t1 = [(0, True), (1, True), (2, True)] + [(l, False) for l in range(3, 8)]
    t2 = [(l, True) for l in range(5)] + [(l, False) for l in range(5, 8)]
    t3 = [(0, True), (2, False), (3, False)]           # level 1: dense, 912 680 entries > 128 * 4096 -- atomic
    assert list(np.diff(_table(T1)[0])[:3]) == [736, 4920, 27000] and list(np.diff(_table(T1)[0])[3:]) == [32768] * 5
    assert list(np.diff(_table(T3)[0])) == [274632, 912680, 1 << 20, 1 << 20] and int(_table(T3)[0][-1]) == 3284464
    for B in (16384, 16421):
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', T1, B) == expect(T1, B, t1)
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', T2, B) == expect(T2, B, t2)
        assert _query(capi, 'ngp_grid_backward_workspace_bytes', T3, B) == expect(T3, B, t3)
