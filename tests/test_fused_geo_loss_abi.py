"""CPU checks of the fused training step with geometry losses (include/ngp_hip.h ngp_composite_train_geo_loss_backward, fused.GeoLoss,
graph.GraphedTrainStep(geo_loss=)): the entry is declared, exported and bound; host-side validation; the ABI version is
unchanged; the GeoLoss record; and the host logic of the graph stepper on stand-in objects."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'ngp_composite_train_geo_loss_backward'


def test_entry_is_declared_exported_and_bound():
    import _ngp_capi as capi
    text = open(os.path.join(ROOT, 'include', 'ngp_hip.h')).read()
    assert re.search(r'\bint\s+' + ENTRY + r'\s*\(', text)
    assert ENTRY in capi.EXPORTED and hasattr(capi.lib, ENTRY)
    fn = getattr(capi.lib, ENTRY)
    assert fn.argtypes == capi._SIGNATURES[ENTRY] and fn.restype == ctypes.c_int
    plain = capi._SIGNATURES['ngp_composite_train_loss_backward']
    assert len(plain) == 24 and len(fn.argtypes) == 30          # + two lambdas, two inputs, two outputs
    # the plain entry's arguments with (lambda_distortion, lambda_depth, target_depth, depth_weight) after target and (depth_raw, distortion)
    # after depth_out
    f32, vp = ctypes.c_float, ctypes.c_void_p
    assert list(fn.argtypes) == plain[:13] + [f32, f32, vp, vp] + plain[13:17] + [vp, vp] + plain[17:]


def test_abi_version_is_unchanged():
    import _ngp_capi as capi
    assert capi.ABI_VERSION == 11 and capi.lib.ngp_abi_version() == 11


def _call(lib, ptrs, lam=(0.5, 0.0), N=16, ws_bytes=None, bg_mode=1):
    """ptrs: dict of the pointer arguments by name (never dereferenced: validation fails first)"""
    p = ptrs
    if ws_bytes is None:
        ws_bytes = lib.ngp_march_rays_train_workspace_bytes(N)
    return lib.ngp_composite_train_geo_loss_backward(p['sigmas'], p['rgbs'], p['deltas'], p['rays'], 100, N, 1e-4, bg_mode, 1.0, p['bg'], p['nears'],
                                                     p['fars'], p['target'], lam[0], lam[1], p['target_depth'], p['depth_weight'], p['loss_scale'],
                                                     p['weights_sum'], p['image_out'], p['depth_out'], p['depth_raw'], p['distortion'], p['loss'],
                                                     p['ray_err'], p['grad_sigmas'], p['grad_out16'], p['march_workspace'], ws_bytes, None)


REQUIRED = ['sigmas', 'rgbs', 'deltas', 'rays', 'nears', 'fars', 'target', 'weights_sum', 'image_out', 'depth_out', 'depth_raw', 'distortion',
            'ray_err', 'grad_sigmas', 'grad_out16', 'march_workspace']
OPTIONAL = ['bg', 'target_depth', 'depth_weight', 'loss_scale', 'loss']


def test_host_validation():
    import _ngp_capi as capi
    lib = capi.lib
    one = ctypes.c_void_p(256)
    full = {k: one for k in REQUIRED}
    full.update({k: None for k in OPTIONAL})
    for name in REQUIRED:
        assert _call(lib, dict(full, **{name: None})) == 1, name
        msg = lib.ngp_last_error()
        assert b'composite_train_geo_loss_backward' in msg and b'NULL' in msg, (name, msg)
    nan, inf = float('nan'), float('inf')
    for lam in [(-1.0, 0.0), (0.0, -1e-3), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, inf)]:
        assert _call(lib, dict(full, target_depth=one), lam=lam) == 1, lam
        msg = lib.ngp_last_error()
        assert b'composite_train_geo_loss_backward' in msg and b'lambda' in msg, (lam, msg)
    assert _call(lib, full, lam=(0.0, 0.25)) == 1                  # depth supervision without a target
    msg = lib.ngp_last_error()
    assert b'composite_train_geo_loss_backward' in msg and b'target_depth' in msg
    need = lib.ngp_march_rays_train_workspace_bytes(16)
    for short in (0, 256, need - 1):
        assert _call(lib, full, ws_bytes=short) == 1
        msg = lib.ngp_last_error()
        assert b'composite_train_geo_loss_backward' in msg and b'group tickets' in msg
    assert _call(lib, full, bg_mode=0) == 1 and b'composite_train_geo_loss_backward' in lib.ngp_last_error()
    assert _call(lib, full, bg_mode=2) == 1 and b'composite_train_geo_loss_backward' in lib.ngp_last_error()   # per-ray mode without bg
    # N == 0 is a no-op, whatever the pointers
    assert _call(lib, {k: None for k in REQUIRED + OPTIONAL}, N=0, ws_bytes=0) == 0


def test_geo_loss_record_validates():
    from fused import GeoLoss
    g = GeoLoss()
    assert g == (0.0, 0.0, None, None) and g.lambda_distortion == 0.0 and g.lambda_depth == 0.0
    g = GeoLoss(lambda_distortion=1, lambda_depth=0)
    assert isinstance(g.lambda_distortion, float) and g.lambda_distortion == 1.0
    z = torch.zeros(8)
    g = GeoLoss(0.5, 0.25, z, depth_weight=z)
    assert g.target_depth is z and g.depth_weight is z and g._replace(lambda_depth=0.0).lambda_depth == 0.0
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            GeoLoss(lambda_distortion=bad)
        with pytest.raises(ValueError):
            GeoLoss(lambda_depth=bad, target_depth=z)
    with pytest.raises(ValueError, match='target_depth'):
        GeoLoss(lambda_depth=0.1)
    with pytest.raises(TypeError):
        GeoLoss(lambda_distortion=torch.tensor(0.1))                # a device scalar cannot be baked into a launch
    with pytest.raises(TypeError):
        GeoLoss(lambda_distortion='0.1')
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, 1), torch.zeros(16)[::2], [0.0] * 8):
        with pytest.raises(ValueError):
            GeoLoss(0.0, 0.1, bad)
        with pytest.raises(ValueError):
            GeoLoss(0.0, 0.0, None, bad)


def test_iteration_entry_points_take_geo_loss():
    import inspect
    import fused
    for fn in (fused.fused_train_iteration, fused.fused_train_iteration_split, fused._train_iteration_rest):
        p = inspect.signature(fn).parameters
        assert 'geo_loss' in p and p['geo_loss'].default is None, fn.__name__
    # a GeoLoss needs the one-launch compositor: refused before anything is launched
    default = fused.USE_FUSED_COMPOSITE
    try:
        fused.USE_FUSED_COMPOSITE = False
        with pytest.raises(RuntimeError, match='USE_FUSED_COMPOSITE'):
            fused._train_iteration_rest(None, None, None, None, None, None, None, None, geo_loss=fused.GeoLoss(0.1))
    finally:
        fused.USE_FUSED_COMPOSITE = default


def _stand_in_step(**attrs):
    asked = []
    m = types.SimpleNamespace(training=True, bg_radius=0, _fused_render_ok=lambda *a, **k: asked.append(a) or True)
    step = types.SimpleNamespace(direct=True, model=m, rays_o=torch.zeros(1, 8, 3), rays_d=torch.zeros(1, 8, 3), autocast_dtype=torch.float16,
                                 render_kwargs={'bg_color': 1}, **attrs)
    return step, asked


def test_direct_path_accepts_geo_loss_and_still_declines_geo_renders():
    """host logic only, on the stand-ins of tests/test_composite_geo_abi.py::test_direct_and_fused_paths_decline_geo"""
    from fused import GeoLoss
    from graph import GraphedTrainStep
    step, asked = _stand_in_step(geo_loss=GeoLoss(lambda_distortion=0.01))
    assert GraphedTrainStep._direct_ok(step) is True and len(asked) == 1
    step.render_kwargs = {'bg_color': 1, 'geo': True}
    assert GraphedTrainStep._direct_ok(step) is False and len(asked) == 1   # declined before the renderer is asked
    step.render_kwargs = {'bg_color': 1, 'staged': True}
    assert GraphedTrainStep._direct_ok(step) is False and len(asked) == 1
    # the geo_loss travels to the iteration through _iteration_args (the stepper always has the field: None without the term)
    opt = types.SimpleNamespace(scalars=torch.zeros(8))
    for geo in (GeoLoss(lambda_distortion=0.01), None):
        s = types.SimpleNamespace(model=types.SimpleNamespace(aabb_train=None), render_kwargs={'bg_color': 1}, optimizer=opt, rays_o=1, rays_d=2,
                                  target=3, counter=torch.zeros(16, 2), captured_capacity=4096, table_fused=False, _overwrites_table=lambda: True,
                                  geo_loss=geo)
        args, kwargs = GraphedTrainStep._iteration_args(s, False)
        assert kwargs['geo_loss'] is geo and args[1:4] == (1, 2, 3)


class _Opt:
    flat_grad16 = torch.zeros(4)


def test_graphed_step_rejects_what_it_cannot_serve():
    from fused import GeoLoss
    from graph import GraphedTrainStep, mse_loss
    model = torch.nn.Linear(2, 2)
    z = torch.zeros(8)
    ok = GraphedTrainStep(model, _Opt(), None, 8, {'bg_color': 1}, geo_loss=GeoLoss(lambda_distortion=0.01))
    assert ok.geo_loss.lambda_distortion == 0.01 and ok.direct
    assert GraphedTrainStep(model, _Opt(), None, 8, {'bg_color': 1}).geo_loss is None
    with pytest.raises(ValueError, match='lambda_depth'):
        GraphedTrainStep(model, _Opt(), None, 8, {'bg_color': 1}, geo_loss=GeoLoss(0.01, 0.1, z))
    with pytest.raises(TypeError):
        GraphedTrainStep(model, _Opt(), None, 8, {'bg_color': 1}, geo_loss=(0.01, 0.0, None, None))
    # not eligible for the autograd-free iteration: raise instead of training without the term
    for kw in (dict(direct=False), dict(loss_fn=lambda out, t: mse_loss(out, t))):
        with pytest.raises(ValueError, match='autograd-free'):
            GraphedTrainStep(model, _Opt(), None, 8, {'bg_color': 1}, geo_loss=GeoLoss(0.01), **kw)
    for rk in ({'geo': True}, {'staged': True}):
        with pytest.raises(ValueError, match='autograd-free'):
            GraphedTrainStep(model, _Opt(), None, 8, dict(rk, bg_color=1), geo_loss=GeoLoss(0.01))
    with pytest.raises(ValueError, match='autograd-free'):
        GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1), None, 8, {'bg_color': 1}, geo_loss=GeoLoss(0.01))
    # ... and a model that turns out not to be eligible when the graphs are about to be captured
    ok._direct_ok = lambda: False
    with pytest.raises(RuntimeError, match='geo_loss'):
        ok._geo_loss_needs_direct()
    ok.geo_loss = None
    ok._geo_loss_needs_direct()
