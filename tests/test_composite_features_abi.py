"""CPU checks of the feature compositor (include/ngp_hip.h ngp_composite_rays_train_features_forward / _backward and their fp64 twins;
raymarching.composite_rays_train_features): declared, exported and bound; the ABI version unchanged; host-side validation;
the Python surface; the fused / direct training paths decline aux and the eval / staged / sharded renders refuse it (host logic on stand-in
objects); and the closed-form backward of tests/composite_features_cases.py against autograd of the definition in float64."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import composite_features_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'ngp_composite_rays_train_features_forward': 11, 'ngp_composite_rays_train_features_backward': 14,
           'ngp_composite_rays_train_features_forward_f64': 10, 'ngp_composite_rays_train_features_backward_f64': 13}


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name, n_args in ENTRIES.items():
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        fn = getattr(capi.lib, name)
        assert fn.argtypes == capi._SIGNATURES[name] and fn.restype == ctypes.c_int and len(fn.argtypes) == n_args
    block = text[text.index('composite arbitrary per-sample feature channels'):text.index('int ngp_composite_rays_train_features_forward(')]
    assert 'EXTENSION' in text[text.index('composite arbitrary per-sample feature channels') - 40:][:60]
    assert 'pre-zeroes' in block and 'grad_sigmas[offset+i]' in block and 'NGP_F16' in block
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        assert name in table, name


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_pybind_table_is_untouched_and_the_op_is_exported():
    import raymarching
    assert 'composite_rays_train_features' in raymarching.raymarching.__all__ and callable(raymarching.composite_rays_train_features)
    from raymarching import backend
    assert callable(backend.composite_rays_train_features_forward) and callable(backend.composite_rays_train_features_backward)
    assert not hasattr(backend._backend, 'composite_rays_train_features_forward')   # the reference's table of callables stays the reference's
    doc = raymarching.raymarching._composite_rays_train_features.__doc__
    assert 'weights_sum' in doc and 'expectation' in doc


def test_host_validation():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    f32, f16 = capi.NGP_F32, capi.NGP_F16

    def fwd(suffix, p, C=5, dtype=f32, M=64, N=4):
        fn = getattr(lib, 'ngp_composite_rays_train_features_forward' + suffix)
        return fn(p[0], p[1], p[2], p[3], M, N, C, 1e-4, p[4], None) if suffix else fn(p[0], p[1], p[2], p[3], M, N, C, 1e-4, dtype, p[4], None)

    def bwd(suffix, p, C=5, dtype=f32, M=64, N=4):
        fn = getattr(lib, 'ngp_composite_rays_train_features_backward' + suffix)
        return fn(*p[:6], M, N, C, 1e-4, p[6], p[7], None) if suffix else fn(*p[:6], M, N, C, 1e-4, dtype, p[6], p[7], None)

    for suffix in ('', '_f64'):
        for call, n_ptr, name in ((fwd, 5, 'forward'), (bwd, 8, 'backward')):
            entry = ('composite_rays_train_features_' + name + suffix).encode()
            assert call(suffix, [one] * n_ptr, M=0, N=0) == 0 and call(suffix, [None] * n_ptr, M=0, N=4) == 0   # N == 0 or M == 0: a no-op
            for i in range(n_ptr):
                p = [one] * n_ptr
                p[i] = None
                assert call(suffix, p) == 1, (suffix, name, i)
                assert entry + b': NULL tensor' in lib.ngp_last_error()
            for C in (0, 257):
                assert call(suffix, [one] * n_ptr, C=C) == 1
                assert entry + b':' in lib.ngp_last_error() and f'C = {C}'.encode() in lib.ngp_last_error()
            if not suffix:
                for dtype in (capi.NGP_F64, 7, -1):
                    assert call(suffix, [one] * n_ptr, dtype=dtype) == 1
                    assert entry + b':' in lib.ngp_last_error() and b'feat_dtype' in lib.ngp_last_error()
                assert f16 == 1 and f32 == 0


def test_direct_and_fused_paths_decline_aux_and_other_renders_refuse_it():
    """host logic only, on stand-ins that are eligible in every other respect"""
    from graph import GraphedTrainStep
    from nerf.renderer import NeRFRenderer
    import ddp
    aux = lambda x, d, s, c: c
    rays = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=(128, 3), device='cpu')
    model = types.SimpleNamespace(fused=True, mean_count=4096, bg_radius=0, _fused_ok=lambda x, d: True)
    assert NeRFRenderer._fused_render_ok(model, rays, rays, 1, False) is True
    assert NeRFRenderer._fused_render_ok(model, rays, rays, 1, False, aux=None) is True
    assert NeRFRenderer._fused_render_ok(model, rays, rays, 1, False, aux=aux) is False
    asked = []
    m = types.SimpleNamespace(training=True, bg_radius=0, _fused_render_ok=lambda *a, **k: asked.append(a) or True)
    step = types.SimpleNamespace(direct=True, model=m, rays_o=torch.zeros(1, 8, 3), rays_d=torch.zeros(1, 8, 3), autocast_dtype=torch.float16,
                                 render_kwargs={'bg_color': 1, 'aux': None})
    assert GraphedTrainStep._direct_ok(step) is True and len(asked) == 1
    step.render_kwargs = {'bg_color': 1, 'aux': aux}
    assert GraphedTrainStep._direct_ok(step) is False and len(asked) == 1   # declined before the renderer is asked

    o = torch.zeros(1, 8, 3)
    evaluating = types.SimpleNamespace(training=False, cuda_ray=True)
    evaluating.run_cuda = functools.partial(NeRFRenderer.run_cuda, evaluating)
    with pytest.raises(NotImplementedError, match='aux'):
        NeRFRenderer.render(evaluating, o, o, aux=aux)
    training = types.SimpleNamespace(training=True, cuda_ray=True)
    with pytest.raises(NotImplementedError, match='aux'):
        NeRFRenderer.render(training, o, o, staged=True, aux=aux)
    with pytest.raises(NotImplementedError, match='aux'):
        NeRFRenderer.render(types.SimpleNamespace(training=True, cuda_ray=False), o, o, aux=aux)
    with pytest.raises(NotImplementedError, match='aux'):
        ddp.render_sharded(training, o, o, rank=0, world=2, aux=aux)


@pytest.mark.parametrize('early', [True, False])
def test_closed_form_matches_the_definition_in_float64(early):
    dead = F.dead_rows(early)
    assert dead.sum() > (600 if early else 100)
    for C in F.CHANNELS:
        ref, got = F.definition(early, C), F.closed_form(early, C, torch.float64)
        for key in F.KEYS:
            assert got[key].shape == ref[key].shape
            assert np.abs(got[key] - ref[key]).max() <= 1e-12, (C, key)
        assert np.abs(ref['grad_sigmas']).max() > 1e-3 and np.abs(ref['out']).max() > 1e-2
        assert (ref['grad_sigmas'][dead] == 0).all() and (ref['grad_feats'][dead] == 0).all()
        for name in ('empty', 'overflow'):
            assert (ref['out'][F.PERM[[n for n, _ in F.RAYS].index(name)]] == 0).all()
        # the bound of the fp32 kernels is neither vacuous nor zero
        for key in F.KEYS:
            bound, err = F.yardstick(early, C, key)
            assert 0 < err < 1e-5 and bound < 1e-4 * max(1.0, float(np.abs(ref[key]).max())), (C, key, err, bound)
