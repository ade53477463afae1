"""CPU checks of the inference loop's feature compositor (include/ngp_hip.h ngp_composite_rays_features / ngp_composite_rays_features_dev;
raymarching.composite_rays_features; render(aux_infer=...)): declared, exported and bound with the ABI version unchanged;
host-side validation before any device work; the Python surface; and where the renderers refuse aux_infer (host logic on stand-in objects)."""
import ctypes
import functools
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'ngp_composite_rays_features': 12, 'ngp_composite_rays_features_dev': 14}


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name, n_args in ENTRIES.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        fn = getattr(capi.lib, name)
        assert fn.argtypes == capi._SIGNATURES[name] and fn.restype == ctypes.c_int and len(fn.argtypes) == n_args
    start = text.index('caller-defined per-sample channels in the inference loop')
    block = text[start:text.index('int ngp_composite_rays_features(')]
    assert 'EXTENSION' in text[start - 40:start]
    for word in ('BEFORE', 'NGP_F16', 'Only out', 'n_step_cap > 1024'):
        assert word in block, word
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert name in table, name
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_the_op_is_exported_and_the_pybind_table_is_untouched():
    import raymarching
    assert 'composite_rays_features' in raymarching.raymarching.__all__ and callable(raymarching.composite_rays_features)
    from raymarching import backend
    assert callable(backend.composite_rays_features) and callable(backend.composite_rays_features_dev)
    assert not hasattr(backend._backend, 'composite_rays_features')   # the reference's table of callables stays the reference's
    doc = raymarching.composite_rays_features.__doc__
    assert 'before composite_rays' in doc and 'in place' in doc and 'float16' in doc


def _host(p, n_alive=61, n_step=4, C=5, dtype=0):
    import _ngp_capi as capi
    return capi.lib.ngp_composite_rays_features(n_alive, n_step, 0.01, p[0], p[1], p[2], p[3], p[4], C, dtype, p[5], None)


def _dev(p, alive_bound=61, cap=0, C=5, dtype=0):
    import _ngp_capi as capi
    return capi.lib.ngp_composite_rays_features_dev(p[0], alive_bound, 4096, cap, 0.01, p[1], p[2], p[3], p[4], p[5], C, dtype, p[6], None)


def test_host_validation_needs_no_gpu():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    for call, n_ptr, entry in ((_host, 6, b'composite_rays_features'), (_dev, 7, b'composite_rays_features_dev')):
        for i in range(n_ptr):
            p = [one] * n_ptr
            p[i] = None
            assert call(p) == 1, (entry, i)
            assert entry + b': NULL tensor' in lib.ngp_last_error()
        for C in (0, 257, 1 << 20):
            assert call([one] * n_ptr, C=C) == 1
            assert entry + b':' in lib.ngp_last_error() and f'C = {C}'.encode() in lib.ngp_last_error()
        for dtype in (capi.NGP_F64, 7, -1):
            assert call([one] * n_ptr, dtype=dtype) == 1
            assert entry + b':' in lib.ngp_last_error() and b'feat_dtype' in lib.ngp_last_error()
    assert capi.NGP_F16 == 1 and capi.NGP_F32 == 0
    assert _dev([one] * 7, cap=1025) == 1 and b'n_step_cap' in lib.ngp_last_error()
    assert _dev([one] * 7, alive_bound=0, cap=1025) == 1          # decided before the zero-count return
    # a launch that would need more than 2^32 lanes is refused, not wrapped
    assert _host([one] * 6, n_alive=1 << 27, C=64) == 1 and b'do not fit one launch' in lib.ngp_last_error()


def test_zero_counts_launch_nothing():
    one = ctypes.c_void_p(256)
    assert _host([one] * 6, n_alive=0) == 0 and _host([None] * 6, n_alive=0) == 0
    assert _dev([one] * 7, alive_bound=0) == 0 and _dev([None] * 7, alive_bound=0, cap=64) == 0
    for dtype in (0, 1):
        for C in (1, 64, 65, 256):
            assert _host([one] * 6, n_alive=0, C=C, dtype=dtype) == 0


def test_the_operator_refuses_float64_and_bad_shapes_before_the_device():
    import raymarching
    f = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    alive = torch.arange(4, dtype=torch.int32)
    for bad in range(5):
        args = [f(8), f(8, 3), f(8, 2), f(4), f(4, 3)]
        args[bad] = args[bad].double()
        with pytest.raises(TypeError, match='composite_rays_features'):
            raymarching.composite_rays_features(4, 2, alive, *args)
    with pytest.raises(RuntimeError, match='composite_rays_features: feats must be'):
        raymarching.composite_rays_features(4, 2, alive, f(8), f(7, 3), f(8, 2), f(4), f(4, 3))     # fewer rows than n_alive * n_step
    with pytest.raises(RuntimeError, match='composite_rays_features: feats must be'):
        raymarching.composite_rays_features(4, 2, alive, f(8), f(8, 3), f(8, 2), f(4), f(4, 5))     # C of feats != C of out
    with pytest.raises(RuntimeError, match='out must be'):
        raymarching.composite_rays_features(4, 2, alive, f(8), f(8, 3, dtype=torch.float16), f(8, 2), f(4), f(4, 3, dtype=torch.float16))
    with pytest.raises(RuntimeError, match='CUDA tensor'):   # a well-formed call reaches the backend, which wants device tensors: no CPU fall-back
        raymarching.composite_rays_features(4, 2, alive, f(8), f(8, 3), f(8, 2), f(4), f(4, 3))


def test_renders_that_refuse_aux_infer():
    """host logic only, on stand-ins"""
    from nerf.renderer import NeRFRenderer
    import ddp
    fn = lambda x, d, s, c: c
    o = torch.zeros(1, 8, 3)
    training = types.SimpleNamespace(training=True, cuda_ray=True)
    training.run_cuda = functools.partial(NeRFRenderer.run_cuda, training)
    with pytest.raises(ValueError, match=r'aux=fn'):
        NeRFRenderer.render(training, o, o, aux_infer=fn)
    for mode in (True, False):
        with pytest.raises(NotImplementedError, match='aux_infer'):
            NeRFRenderer.render(types.SimpleNamespace(training=mode, cuda_ray=False), o, o, aux_infer=fn)
        with pytest.raises(NotImplementedError, match='aux_infer'):
            NeRFRenderer.render(types.SimpleNamespace(training=mode, cuda_ray=False), o, o, staged=True, aux_infer=fn)
        with pytest.raises(NotImplementedError, match='aux_infer'):
            ddp.render_sharded(types.SimpleNamespace(training=mode, cuda_ray=True), o, o, rank=0, world=2, aux_infer=fn)
    # aux= keeps raising in eval, and now says where to go
    evaluating = types.SimpleNamespace(training=False, cuda_ray=True)
    evaluating.run_cuda = functools.partial(NeRFRenderer.run_cuda, evaluating)
    with pytest.raises(NotImplementedError, match='aux_infer=fn'):
        NeRFRenderer.render(evaluating, o, o, aux=fn)


def test_the_callable_contract_is_checked_per_call():
    from nerf.renderer import NeRFRenderer
    check = NeRFRenderer._aux_infer_feats
    x = torch.zeros(128, 3)
    s = torch.zeros(128)
    frame = {'out': None}
    feats = check(lambda x, d, s, c: torch.ones(128, 7, dtype=torch.float16), frame, x, x, s, x, 40)
    assert feats.dtype == torch.float16 and feats.shape == (128, 7)
    assert frame['out'].shape == (40, 7) and frame['out'].dtype == torch.float32 and not frame['out'].any()
    first = frame['out']
    check(lambda x, d, s, c: torch.ones(128, 7, dtype=torch.float16), frame, x, x, s, x, 40)
    assert frame['out'] is first
    with pytest.raises(ValueError, match='same C and dtype'):
        check(lambda x, d, s, c: torch.ones(128, 8, dtype=torch.float16), frame, x, x, s, x, 40)
    with pytest.raises(ValueError, match='same C and dtype'):
        check(lambda x, d, s, c: torch.ones(128, 7), frame, x, x, s, x, 40)
    for bad in (torch.ones(127, 7), torch.ones(128), torch.ones(128, 0), torch.ones(128, 257), None):
        with pytest.raises(ValueError, match='must return a'):
            check(lambda x, d, s, c: bad, {'out': None}, x, x, s, x, 40)
    with pytest.raises(ValueError, match='float32 or float16'):
        check(lambda x, d, s, c: torch.ones(128, 3, dtype=torch.float64), {'out': None}, x, x, s, x, 40)
    w = torch.ones(3, 2, requires_grad=True)
    assert not check(lambda x, d, s, c: c @ w, {'out': None}, x, x, s, x, 40).requires_grad      # no gradient graph
