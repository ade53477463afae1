"""CPU checks of the geometry compositor (include/ngp_hip.h ngp_composite_rays_train_geo_forward / _backward and their fp64 twins;
raymarching.composite_rays_train_geo): declared, exported and bound; the ABI version unchanged; host-side validation; the
Python surface; the fused / direct training paths decline geo=True (host logic on stand-in objects); and the shared cases of
tests/composite_geo_cases.py themselves -- the ray table's conditions and the O(K) formulas against the O(K^2) definition in float64."""
import ctypes
import os
import re
import types

import numpy as np
import torch

import composite_geo_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['ngp_composite_rays_train_geo_forward', 'ngp_composite_rays_train_geo_backward', 'ngp_composite_rays_train_geo_forward_f64',
           'ngp_composite_rays_train_geo_backward_f64']


def test_entries_are_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    for name in ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
        assert name in capi.EXPORTED and hasattr(capi.lib, name)
        fn = getattr(capi.lib, name)
        assert fn.argtypes == capi._SIGNATURES[name] and fn.restype == ctypes.c_int
        assert len(fn.argtypes) == (18 if 'backward' in name else 12)
    # the comment of the new block cites what it extends
    block = text[text.index('EXTENSION of composite_rays_train_forward'):text.index('int ngp_composite_rays_train_geo_forward(')]
    assert 'raymarching.cu:501-577, 602-682' in block and 'loss.py::EffDistLoss' in block


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def test_pybind_table_is_untouched_and_the_op_is_exported():
    import raymarching
    assert 'composite_rays_train_geo' in raymarching.raymarching.__all__ and callable(raymarching.composite_rays_train_geo)
    from raymarching import backend
    assert callable(backend.composite_rays_train_geo_forward) and callable(backend.composite_rays_train_geo_backward)
    assert not hasattr(backend._backend, 'composite_rays_train_geo_forward')   # the reference's table of callables stays the reference's


def test_host_validation():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)  # never dereferenced: validation fails first
    for suffix in ('', '_f64'):
        fwd, bwd = getattr(lib, 'ngp_composite_rays_train_geo_forward' + suffix), getattr(lib, 'ngp_composite_rays_train_geo_backward' + suffix)
        for i in range(8):  # sigmas, rgbs, deltas, rays, weights_sum, depth, image, distortion
            p = [one] * 8
            p[i] = None
            assert fwd(p[0], p[1], p[2], p[3], 64, 4, 1e-4, p[4], p[5], p[6], p[7], None) == 1, (suffix, i)
            assert b'composite_rays_train_geo_forward' + suffix.encode() + b': NULL tensor' in lib.ngp_last_error()
        for i in range(4, 14):  # the four upstream gradients (0..3) may be NULL; the saved tensors and the two outputs may not
            p = [one] * 14
            p[i] = None
            assert bwd(*p[:12], 64, 4, 1e-4, p[12], p[13], None) == 1, (suffix, i)
            assert b'composite_rays_train_geo_backward' + suffix.encode() + b': NULL tensor' in lib.ngp_last_error()
        # N == 0 is a no-op, whatever the pointers
        assert fwd(None, None, None, None, 0, 0, 1e-4, None, None, None, None, None) == 0
        assert bwd(*[None] * 12, 0, 0, 1e-4, None, None, None) == 0


def test_direct_and_fused_paths_decline_geo():
    """host logic only: GraphedTrainStep._direct_ok and NeRFRenderer._fused_render_ok on stand-ins that are eligible in every other respect"""
    from graph import GraphedTrainStep
    from nerf.renderer import NeRFRenderer
    rays = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=(128, 3), device='cpu')
    model = types.SimpleNamespace(fused=True, mean_count=4096, bg_radius=0, _fused_ok=lambda x, d: True)
    assert NeRFRenderer._fused_render_ok(model, rays, rays, 1, False) is True
    assert NeRFRenderer._fused_render_ok(model, rays, rays, 1, False, geo=False) is True
    assert NeRFRenderer._fused_render_ok(model, rays, rays, 1, False, geo=True) is False
    asked = []
    m = types.SimpleNamespace(training=True, bg_radius=0, _fused_render_ok=lambda *a, **k: asked.append(a) or True)
    step = types.SimpleNamespace(direct=True, model=m, rays_o=torch.zeros(1, 8, 3), rays_d=torch.zeros(1, 8, 3), autocast_dtype=torch.float16,
                                 render_kwargs={'bg_color': 1})
    assert GraphedTrainStep._direct_ok(step) is True and len(asked) == 1
    step.render_kwargs = {'bg_color': 1, 'geo': False}
    assert GraphedTrainStep._direct_ok(step) is True and len(asked) == 2
    step.render_kwargs = {'bg_color': 1, 'geo': True}
    assert GraphedTrainStep._direct_ok(step) is False and len(asked) == 2   # declined before the renderer is asked


def test_ray_table_meets_its_conditions():
    for early in (True, False):
        t, ref = C.ray_table(early), C.table_reference(early)
        rays, live = t['rays'], dict(zip(C.NAMES, ref['live']))
        assert sorted(rays[:, 0].tolist()) == list(range(len(C.RAYS))) and rays[:, 0].tolist() != list(range(len(C.RAYS)))   # shuffled rows
        assert [int(n) for n in rays[:, 2]] == [0, 1, 63, 64, 65, 130, 300, 300, 200, 300] and 1500 <= C.M <= 1700
        assert (t['deltas'][t['used']:] == 0).all() and (t['deltas'][:t['used']] > 0).all()
        over = rays[C.NAMES.index('overflow')]
        assert over[1] < C.M < over[1] + over[2] and live['overflow'] == 0 and live['empty'] == 0
        if early:
            assert 1 <= live['saturating'] < 64          # stops inside the first row
            assert live['boundary'] == 64                # T crosses T_thresh with sample 63: the first row is all live, the second never runs
            assert live['long'] == 300 and live['three rows'] == 130
        else:
            assert [live[n] for n in C.NAMES] == [0, 1, 63, 64, 65, 130, 300, 300, 200, 0]
            assert (ref['weights_sum'] < 0.9).all()      # no sample near the T_thresh discontinuity
        # empty and overflowing rays leave zero rows
        for name in ('empty', 'overflow'):
            row = rays[C.NAMES.index(name), 0]
            assert ref['weights_sum'][row] == 0 and ref['depth'][row] == 0 and ref['distortion'][row] == 0 and (ref['image'][row] == 0).all()


def test_prefix_form_and_closed_form_backward_match_the_definition_in_float64():
    """the O(K) distortion with two exclusive prefixes and the single-sweep backward (G = 2 L) against the O(K^2) definition and autograd"""
    for early in (True, False):
        t, ref = C.ray_table(early), C.table_reference(early)
        got = C.prefix_form(t['sigmas'], t['rgbs'], t['deltas'], t['rays'], C.upstream(), torch.float64)
        for key in ('weights_sum', 'depth', 'image', 'distortion', 'grad_sigmas', 'grad_rgbs'):
            scale = max(1.0, float(np.abs(ref[key]).max()))
            assert np.abs(got[key] - ref[key]).max() <= 1e-13 * scale, key
        assert np.abs(ref['grad_sigmas']).max() > 1e-3 and np.abs(ref['distortion']).max() > 1e-2
        # rows no ray composites get no gradient: behind an early stop, the overflowing ray's, the padding
        mask = np.zeros(C.M, bool)
        for (_, off, _), k in zip(t['rays'], ref['live']):
            mask[off:off + k] = True
        assert (ref['grad_sigmas'][~mask] == 0).all() and (ref['grad_rgbs'][~mask] == 0).all() and (ref['grad_sigmas'][mask] != 0).all()
