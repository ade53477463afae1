"""GPU checks of the inference loop's feature compositor: ngp_composite_rays_features / ngp_composite_rays_features_dev
(k_composite_rays_feat, include/ngp_hip.h) at the C ABI on the tables of tests/render_features_cases.py, and render(aux_infer=...) on top
(DESIGN.md 3.12).

Tolerance of `out` against the float64 definition: 4 x (error of the float32 model of the same statements, same inputs) + 1e-7 x (largest
reference magnitude), per (n_step, C); everything else is exact: the fp16 call against the fp32 call on the up-cast values, the colour and
the weight channel against ngp_composite_rays' image and weights_sum, the `_dev` entry against the host entry, two runs against each other,
and every "unchanged" claim.  The tables put NaN into every feature row at or behind a ray's break: a read behind the break shows in `out`.
Every test prints its figures before it asserts (pytest -s).

Measured on MI355X, smallest .. largest over n_step in N_STEPS and the channel counts (the float32 model's exponential is numpy's fp32 exp;
the exp2 restatement render_loop_cases offers was not needed):
                                  kernel error          float32 model error    bound                  kernel error / bound
    fp32, 9 channel counts        4.0e-08 .. 6.6e-07    5.6e-08 .. 8.2e-07     3.2e-07 .. 3.4e-06     0.11 .. 0.27
    fp16, 4 channel counts        6.1e-08 .. 8.2e-07    8.2e-08 .. 7.0e-07     4.3e-07 .. 3.0e-06     0.11 .. 0.28
    3 calls of 4, C = 3, 33, 130  2.0e-07 .. 2.9e-07    2.0e-07 .. 2.9e-07     9.8e-07 .. 1.3e-06     0.17 .. 0.22
The whole file (146 cases) takes about 4 s."""
import numpy as np
import pytest
import torch

import render_features_cases as F
import render_loop_cases as L

pytestmark = pytest.mark.gpu

CHANNELS_F32 = (1, 3, 5, 21, 33, 64, 65, 130, 256)
CHANNELS_F16 = (3, 22, 64, 65)
# (n_total, cap) from which the device derives each n_step of the tables for the 61 rays of the list, with the two caps of L.LADDER
DEV_N_STEP = {1: (61, 0), 2: (130, 0), 3: (200, 0), 8: (4096, 0), 13: (800, 64), 64: (4096, 64)}


def _capi():
    import _ngp_capi as capi
    return capi


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def p(t):
    return t.data_ptr()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape
    view = torch.int16 if a.dtype == torch.float16 else torch.int32
    return torch.equal(a.view(view), b.view(view))


def _upload(call, feats, out0, rays_alive=None, rows=None):
    """one call's tensors on the device.  `rows` > n_alive * n_step: the sample buffers are that long and NaN behind the list's rows"""
    n = call['n_alive'] * call['n_step']
    sg, rg, de = call['sigmas'].reshape(-1), call['rgbs'].reshape(-1, 3), call['deltas'].reshape(-1, 2)
    ft = feats.reshape(n, -1)
    if rows is not None and rows > n:
        tail = lambda a: np.concatenate([a, np.full((rows - n,) + a.shape[1:], np.nan, a.dtype)])
        sg, rg, de, ft = tail(sg), tail(rg), tail(de), tail(ft)
    s = {k: cu(call[k].astype(np.float32)) for k in L.KEYS}
    s.update(rays_alive=cu(call['rays_alive'] if rays_alive is None else rays_alive), sigmas=cu(sg), rgbs=cu(rg), deltas=cu(de), feats=cu(ft),
             out=cu(out0.astype(np.float32)))
    return s


def _clone(s):
    return {k: v.clone() for k, v in s.items()}


def _code(t):
    return {torch.float32: _capi().NGP_F32, torch.float16: _capi().NGP_F16}[t.dtype]


def _features(s, n_alive, n_step, T_thresh):
    capi = _capi()
    capi.check(capi.lib.ngp_composite_rays_features(n_alive, n_step, T_thresh, p(s['rays_alive']), p(s['sigmas']), p(s['feats']), p(s['deltas']),
                                                    p(s['weights_sum']), s['out'].shape[1], _code(s['feats']), p(s['out']), capi.stream()))
    torch.cuda.synchronize()


def _features_dev(s, state, alive_bound, n_total, cap, T_thresh):
    capi = _capi()
    capi.check(capi.lib.ngp_composite_rays_features_dev(p(state), alive_bound, n_total, cap, T_thresh, p(s['rays_alive']), p(s['sigmas']), p(s['feats']),
                                                        p(s['deltas']), p(s['weights_sum']), s['out'].shape[1], _code(s['feats']), p(s['out']),
                                                        capi.stream()))
    torch.cuda.synchronize()


def _composite(s, n_alive, n_step, T_thresh):
    capi = _capi()
    capi.check(capi.lib.ngp_composite_rays(n_alive, n_step, T_thresh, p(s['rays_alive']), p(s['rays_t']), p(s['sigmas']), p(s['rgbs']), p(s['deltas']),
                                           p(s['weights_sum']), p(s['depth']), p(s['image']), capi.stream()))
    torch.cuda.synchronize()


def _only_out_changed(s, before, table):
    for key in s:
        if key != 'out':
            assert _same_bits(s[key], before[key]), key
    outside = cu(table['outside'].astype(np.int64))
    assert _same_bits(s['out'][outside], before['out'][outside])


# ------------------------------------------------------------------------------------------------
# 1. the definition
# ------------------------------------------------------------------------------------------------
def _against_the_definition(n_step, C, half):
    t = F.features_table(n_step, C)
    feats = F.table_feats(n_step, C, half)
    assert np.isnan(feats).any() or n_step == 1                                            # the poison is in place
    s = _upload(t, feats, t['out0'])
    before = _clone(s)
    _features(s, t['n_alive'], n_step, t['T_thresh'])
    ref, _ = F.features_reference(n_step, C, half)
    bound, model_err = F.features_bound(n_step, C, half=half)
    got = s['out'].double().cpu().numpy()
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f"composite_rays_features n_step={n_step} C={C} {'fp16' if half else 'fp32'}: kernel error {err:.3e}, float32 model error {model_err:.3e}, "
          f'bound {bound:.3e}, err / bound {err / bound:.3f}')
    assert err <= bound, (n_step, C, half, err, bound)
    _only_out_changed(s, before, t)
    listed = cu(t['rays_alive'].astype(np.int64))
    assert not _same_bits(s['out'][listed], before['out'][listed])
    return s, before


@pytest.mark.parametrize('C', CHANNELS_F32)
@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_fp32_features_match_the_float64_definition(n_step, C):
    _against_the_definition(n_step, C, False)


@pytest.mark.parametrize('C', CHANNELS_F16)
@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_fp16_features_match_the_definition_and_the_fp32_call_on_the_upcast_values(n_step, C):
    s, before = _against_the_definition(n_step, C, True)
    assert s['feats'].dtype == torch.float16
    up = dict(before, feats=before['feats'].float())
    t = F.features_table(n_step, C)
    _features(up, t['n_alive'], n_step, t['T_thresh'])
    assert _same_bits(up['out'], s['out'])


# ------------------------------------------------------------------------------------------------
# 2. the bits of ngp_composite_rays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_colour_and_weight_channels_have_the_bits_of_composite_rays(n_step):
    t = L.composite_table(n_step)
    n = t['n_alive'] * n_step
    colour = _upload(t, t['rgbs'].reshape(n, 3), t['image'])
    ones = _upload(t, np.ones((n, 1), np.float32), t['weights_sum'][:, None])
    before = _clone(colour)
    _features(colour, t['n_alive'], n_step, t['T_thresh'])          # BEFORE the compositor's call on the same rows
    _features(ones, t['n_alive'], n_step, t['T_thresh'])
    _only_out_changed(colour, before, t)
    _composite(colour, t['n_alive'], n_step, t['T_thresh'])
    assert torch.equal(colour['out'], colour['image']) and _same_bits(colour['out'], colour['image'])
    assert torch.equal(ones['out'][:, 0], colour['weights_sum']) and _same_bits(ones['out'][:, 0], colour['weights_sum'])
    assert not torch.equal(colour['image'], before['image'])


# ------------------------------------------------------------------------------------------------
# 3. three consecutive calls
# ------------------------------------------------------------------------------------------------
def _three_calls(C):
    calls, tab = L.multi_call_table(), F.features_multi_table(C)
    lists = L.multi_yardstick()[1]
    s = _upload(calls[0], tab['feats'][0], tab['out0'])
    for i, (call, feats) in enumerate(zip(calls, tab['feats'])):
        assert np.array_equal(s['rays_alive'].cpu().numpy(), call['rays_alive'])   # the compacted list of the kernels' own previous call
        s.update(sigmas=cu(call['sigmas'].reshape(-1)), rgbs=cu(call['rgbs'].reshape(-1, 3)), deltas=cu(call['deltas'].reshape(-1, 2)),
                 feats=cu(feats.reshape(-1, C)))
        _features(s, call['n_alive'], call['n_step'], call['T_thresh'])
        _composite(s, call['n_alive'], call['n_step'], call['T_thresh'])
        assert np.array_equal(s['rays_alive'].cpu().numpy(), lists[i]), i
        s['rays_alive'] = s['rays_alive'][s['rays_alive'] >= 0].contiguous()
    return s['out']


@pytest.mark.parametrize('C', [3, 33, 130])
def test_three_consecutive_calls(C):
    ref, bound, model_err = F.features_multi_bound(C)
    a, b = _three_calls(C), _three_calls(C)
    got = a.double().cpu().numpy()
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f'composite_rays_features, 3 calls of n_step=4, C={C}: kernel error {err:.3e}, float32 model error {model_err:.3e}, bound {bound:.3e}, '
          f'err / bound {err / bound:.3f}')
    assert err <= bound, (C, err, bound)
    assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------
# 4. the device-state entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,half', [(3, False), (65, False), (22, True)])
@pytest.mark.parametrize('alive_bound', [L.N_ALIVE, L.N_ALIVE + 37, 97])
@pytest.mark.parametrize('n_step', L.N_STEPS)
def test_dev_entry_equals_the_host_entry(n_step, alive_bound, C, half):
    t = F.features_table(n_step, C)
    n_total, cap = DEV_N_STEP[n_step]
    assert L.loop_n_step(n_total, L.N_ALIVE, cap) == n_step and cap in {c for _, _, c, _ in L.LADDER}
    # list entries [61, alive_bound): valid ids of rays OUTSIDE the list; sample rows behind the 61 rays': NaN
    full_list = np.concatenate([t['rays_alive'], np.resize(t['outside'], alive_bound - L.N_ALIVE)]).astype(np.int32)
    host = _upload(t, F.table_feats(n_step, C, half), t['out0'], full_list, rows=alive_bound * n_step)
    dev, before = _clone(host), _clone(host)
    _features(host, L.N_ALIVE, n_step, t['T_thresh'])
    state = cu(np.array([L.N_ALIVE, 17], np.int32))
    _features_dev(dev, state, alive_bound, n_total, cap, t['T_thresh'])
    assert state.cpu().tolist() == [L.N_ALIVE, 17]
    assert _same_bits(host['out'], dev['out']) and torch.isfinite(dev['out']).all()
    _only_out_changed(dev, before, t)
    listed = cu(t['rays_alive'].astype(np.int64))
    assert not _same_bits(dev['out'][listed], before['out'][listed])


@pytest.mark.parametrize('cap', [0, 64])
def test_dev_entry_with_a_device_count_of_zero_changes_nothing(cap):
    t = F.features_table(8, 33)
    full_list = np.concatenate([t['rays_alive'], np.resize(t['outside'], 97 - L.N_ALIVE)]).astype(np.int32)
    s = _upload(t, t['feats'], t['out0'], full_list, rows=97 * 8)
    before = _clone(s)
    state = cu(np.array([0, 17], np.int32))
    _features_dev(s, state, 97, 4096, cap, t['T_thresh'])
    for key in s:
        assert _same_bits(s[key], before[key]), key
    assert state.cpu().tolist() == [0, 17]


def test_operator_updates_out_in_place_and_keeps_fp16_under_autocast():
    import raymarching
    t = F.features_table(8, 22)
    s = _upload(t, F.table_feats(8, 22, True), t['out0'])
    want = _clone(s)
    _features(want, t['n_alive'], 8, t['T_thresh'])
    with torch.autocast('cuda', dtype=torch.float16):
        back = raymarching.composite_rays_features(t['n_alive'], 8, s['rays_alive'], s['sigmas'], s['feats'].requires_grad_(False), s['deltas'],
                                                   s['weights_sum'], s['out'], t['T_thresh'])
    assert back is s['out'] and _same_bits(s['out'], want['out'])
    with pytest.raises(TypeError, match='composite_rays_features'):
        raymarching.composite_rays_features(t['n_alive'], 8, s['rays_alive'], s['sigmas'], s['feats'].double(), s['deltas'], s['weights_sum'], s['out'])


# ------------------------------------------------------------------------------------------------
# 5. the renderer
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def frame():
    import oracle  # noqa: F401
    import raymarching
    import synthetic_scene as sc
    from nerf.network_ff import NeRFNetwork
    from oracle.pipeline import OracleNeRF
    dev = torch.device('cuda')
    orc = OracleNeRF(bound=1.0, seed=3, emb_scale=0.5)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    with torch.no_grad():
        model.encoder.embeddings.copy_(torch.from_numpy(orc.embeddings))
        model.sigma_net.weights.copy_(torch.from_numpy(orc.w_sigma))
        model.color_net.weights.copy_(torch.from_numpy(orc.w_color))
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.eval()
    model.density_scale = 40.0
    rng = np.random.default_rng(3)
    o, d = sc.rays_for_pixels(sc.camera_pose(rng), rng.integers(0, sc.RES * sc.RES, 128))
    return model, torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev)


def _render(frame, device_loop=True, **kw):
    model, o, d = frame
    model.device_loop = device_loop
    model._loop_native_pairs = 0
    try:
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
            out = model.render(o, d, staged=True, bg_color=0, perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4, **kw)
        torch.cuda.synchronize()
    finally:
        model.device_loop = True
    return out, model._loop_native_pairs


def test_render_aux_infer(frame):
    plain, pairs = _render(frame)
    assert pairs >= 1 and 'aux' not in plain                       # the plain frame of this model takes the native pair call
    assert float(plain['image'].std()) > 0
    calls = []

    def colours(x, d, s, c):
        calls.append((tuple(x.shape), tuple(d.shape), tuple(s.shape), s.dtype, tuple(c.shape), c.dtype, x.shape[0] % 128))
        return c

    got, pairs = _render(frame, aux_infer=colours)
    assert pairs == 0                                              # a Python callable cannot be issued from C
    assert len(calls) >= 2 and all(c[0] == c[1] == c[4] and c[2] == c[0][:1] and c[3] == c[5] == torch.float32 and c[6] == 0 for c in calls)
    assert got['aux'].shape == (1, 128, 3) and got['aux'].dtype == torch.float32
    assert torch.equal(got['aux'], got['image'])                   # bg_color = 0: the image IS the raw composite of the colours
    depth = lambda r: torch.nan_to_num(r['depth'], nan=-1.0)       # (rays that miss the box carry depth = 0 / 0 on every path)
    assert torch.equal(got['image'], plain['image']) and torch.equal(depth(got), depth(plain))
    host, pairs = _render(frame, device_loop=False, aux_infer=colours)
    assert pairs == 0 and torch.equal(host['aux'], got['aux']) and torch.equal(host['image'], plain['image']) and torch.equal(depth(host), depth(plain))
    print(f"render(aux_infer): {len(calls)} calls, rows {sorted({c[0][0] for c in calls})}")


def test_render_aux_infer_fp16_channels_and_a_callable_that_changes_C(frame):
    seven = lambda x, d, s, c: torch.cat([c, torch.ones_like(c[:, :1]), x], 1).half()
    plain, _ = _render(frame)
    for device_loop in (True, False):
        got, _ = _render(frame, device_loop=device_loop, aux_infer=seven)
        aux = got['aux']
        assert aux.shape == (1, 128, 7) and aux.dtype == torch.float32 and torch.isfinite(aux).all() and float(aux.abs().max()) > 0
        assert torch.equal(got['image'], plain['image'])
        # the colours went through fp16 on their way: close to the image, not its bits; the ones channel is the opacity
        assert float((aux[..., :3] - plain['image']).abs().max()) < 2e-3 and float(aux[..., 3].max()) <= 1.0 + 1e-6
    n = [0]

    def changing(x, d, s, c):
        n[0] += 1
        return c if n[0] == 1 else c[:, :2]

    for device_loop in (True, False):
        n[0] = 0
        with pytest.raises(ValueError, match='same C and dtype'):
            _render(frame, device_loop=device_loop, aux_infer=changing)
    model = frame[0]
    model.train()
    try:
        with pytest.raises(ValueError, match='aux=fn'):
            model.render(frame[1], frame[2], aux_infer=seven)
    finally:
        model.eval()
