"""GPU checks of the geometry compositor raymarching.composite_rays_train_geo (k_composite_train_geo_fwd / _bwd and their fp64 twins;
DESIGN.md 3.9) on the shared ray table of tests/composite_geo_cases.py: fp64 against the O(K^2) definition and autograd (+ gradcheck); fp32
bit-identical to composite_rays_train in everything the two share, the distortion and the full backward inside a yardstick measured from the
float32 rounding of the same formulas on the CPU; the plain backward's zero fill (rows_used) against the pre-zeroed call; depth's gradient (zero through composite_rays_train, as in the reference); determinism;
NeRFRenderer.run_cuda(geo=True).

Figures measured on MI355X (kernel error against the float64 reference, bound = 4 x the CPU float32 error of the same formulas + 1e-7
max|ref|): DESIGN.md 3.9.  The whole file takes about 6 s, 2.4 s of it the gradcheck."""
import numpy as np
import pytest
import torch

import composite_geo_cases as C

pytestmark = pytest.mark.gpu

KEYS = ('weights_sum', 'depth', 'image', 'distortion')


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _inputs(early, dtype):
    t = C.ray_table(early)
    return (cu(t['sigmas'], dtype).requires_grad_(), cu(t['rgbs'], dtype).requires_grad_(), cu(t['deltas'], dtype), cu(t['rays']))


def _run(op, early, dtype, grads=None, keys=KEYS):
    """forward (+ backward with the upstream gradients `grads`) -> dict of outputs and gradients, as float64 numpy"""
    s, c, d, r = _inputs(early, dtype)
    out = dict(zip(keys, op(s, c, d, r, C.T_THRESH)))
    res = {k: v.detach() for k, v in out.items()}
    if grads is not None:
        loss = sum((cu(grads[k], dtype) * out[k]).sum() for k in grads)
        loss.backward()
        res['grad_sigmas'], res['grad_rgbs'] = s.grad, c.grad
    return res


def _np(res):
    return {k: v.double().cpu().numpy() for k, v in res.items()}


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _close(got, want, rel=1e-12):
    """the tolerance of tests/test_gpu_fp64.py::_close"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want)
    bound = rel * np.abs(want) + rel * 1e-2 * max(1.0, float(np.abs(want).max(initial=0.0)))
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), got[bad][:4], want[bad][:4])


def _dead_rows(early):
    t, ref = C.ray_table(early), C.table_reference(early)
    dead = np.ones(C.M, bool)
    for (_, off, _), k in zip(t['rays'], ref['live']):
        dead[off:off + k] = False
    return dead


# ------------------------------------------------------------------------------------------------
# 1. fp64 against the loop reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('early', [True, False])
def test_fp64_forward_and_backward_match_the_definition(early):
    import raymarching
    ref = C.table_reference(early)
    got = _np(_run(raymarching.composite_rays_train_geo, early, torch.float64, C.upstream()))
    for key in KEYS + ('grad_sigmas', 'grad_rgbs'):
        _close(got[key], ref[key])
    dead = _dead_rows(early)
    assert (got['grad_sigmas'][dead] == 0).all() and (got['grad_rgbs'][dead] == 0).all()


def test_fp64_gradcheck_all_four_outputs():
    import raymarching
    assert (C.table_reference(False)['weights_sum'] < 0.9).all()
    s, c, d, r = _inputs(False, torch.float64)
    assert torch.autograd.gradcheck(lambda s_, c_: raymarching.composite_rays_train_geo(s_, c_, d, r, C.T_THRESH), (s, c), nondet_tol=0.0)


# ------------------------------------------------------------------------------------------------
# 2. / 3. fp32
# ------------------------------------------------------------------------------------------------
def test_fp32_forward_shares_its_bits_with_composite_rays_train():
    import raymarching
    geo = _run(raymarching.composite_rays_train_geo, True, torch.float32)
    old = _run(raymarching.composite_rays_train, True, torch.float32, keys=KEYS[:3])
    for key in KEYS[:3]:
        assert _bits_equal(geo[key], old[key]), key


@pytest.mark.parametrize('early', [True, False])
def test_fp32_distortion_within_the_float32_yardstick(early):
    """Measured on MI355X: early=True kernel 2.351e-08, CPU float32 1.427e-07, bound 7.359e-07; early=False kernel 8.380e-08, CPU float32
    5.122e-07, bound 2.214e-06.  (Summed over the weights the op shares bit for bit with composite_rays_train the distortion was 7.388e-07 off
    in both tables -- weights_sum of the 300-sample 'long' ray is 4.5 ulp off -- and missed the first bound: the forward kernel gives the
    distortion log-domain weights of its own)"""
    import raymarching
    ref = C.table_reference(early)
    got = _np(_run(raymarching.composite_rays_train_geo, early, torch.float32))
    bound, cpu_err = C.yardstick(early, 'distortion')
    err = float(np.abs(got['distortion'] - ref['distortion']).max())
    print(f'distortion early={early}: kernel error {err:.3e}, CPU float32 error {cpu_err:.3e}, bound {bound:.3e}')
    assert err <= bound, (err, bound)
    for name in ('empty', 'overflow'):
        assert got['distortion'][C.PERM[C.NAMES.index(name)]] == 0


def test_fp32_backward_without_depth_and_distortion_gradients_shares_its_bits():
    import raymarching
    up = C.upstream()
    plain = {'weights_sum': up['weights_sum'], 'image': up['image']}
    zeros = dict(plain, depth=np.zeros_like(up['depth']), distortion=np.zeros_like(up['distortion']))
    old = _run(raymarching.composite_rays_train, True, torch.float32, plain, keys=KEYS[:3])
    for grads in (plain, zeros):   # absent (NULL pointers) and explicit zero gradients
        geo = _run(raymarching.composite_rays_train_geo, True, torch.float32, grads)
        assert _bits_equal(geo['grad_sigmas'], old['grad_sigmas']) and _bits_equal(geo['grad_rgbs'], old['grad_rgbs'])


def test_fp32_backward_of_all_four_outputs_within_the_float32_yardstick():
    import raymarching
    ref = C.table_reference(False)
    got = _np(_run(raymarching.composite_rays_train_geo, False, torch.float32, C.upstream()))
    for key in ('grad_sigmas', 'grad_rgbs'):
        bound, cpu_err = C.yardstick(False, key)
        err = float(np.abs(got[key] - ref[key]).max())
        print(f'{key}: kernel error {err:.3e}, CPU float32 error {cpu_err:.3e}, bound {bound:.3e}')
        assert err <= bound, (key, err, bound)


def test_fp32_backward_leaves_uncomposited_rows_exactly_zero():
    import raymarching
    got = _np(_run(raymarching.composite_rays_train_geo, True, torch.float32, C.upstream()))
    dead = _dead_rows(True)
    assert dead.sum() > 600   # behind the two early stops, the overflowing ray's rows, the padding
    assert (got['grad_sigmas'][dead] == 0).all() and (got['grad_rgbs'][dead] == 0).all()
    assert (got['grad_sigmas'][~dead] != 0).all()


@pytest.mark.parametrize('bg_mode, with_grad_ws', [(0, True), (2, False)])
@pytest.mark.parametrize('early', [True, False])
def test_fp32_backward_zero_fill_equals_the_prezeroed_call(early, bg_mode, with_grad_ws):
    """ngp_composite_rays_train_backward_ex with rows_used into NaN-filled outputs (the kernel zeroes every row the compositing does not
    reach) against the same call with rows_used = NULL into zero-filled ones: the run-time zero_fill of the sweep's fp32 sink"""
    import _ngp_capi as capi
    t, up, N = C.ray_table(early), C.upstream(), len(C.RAYS)
    f32 = lambda a: cu(a, torch.float32)
    sigmas, rgbs, deltas, rays = f32(t['sigmas']), f32(t['rgbs']), f32(t['deltas']), cu(t['rays'])
    g_ws, g_img = (f32(up['weights_sum']) if with_grad_ws else None), f32(up['image'])
    bg = f32(np.random.default_rng(11).uniform(0, 1, (N, 3))) if bg_mode == 2 else None
    ws, depth, image = (torch.full(s, float('nan'), device='cuda') for s in ((N,), (N,), (N, 3)))
    st = capi.stream()
    capi.check(capi.lib.ngp_composite_rays_train_forward(sigmas.data_ptr(), rgbs.data_ptr(), deltas.data_ptr(), rays.data_ptr(), C.M, N, C.T_THRESH,
                                                         ws.data_ptr(), depth.data_ptr(), image.data_ptr(), st))
    rows_used = torch.tensor([t['used']], dtype=torch.int32, device='cuda')
    got = {}
    for filled in (True, False):
        fill = float('nan') if filled else 0.0
        gs, gc = torch.full((C.M,), fill, device='cuda'), torch.full((C.M, 3), fill, device='cuda')
        capi.check(capi.lib.ngp_composite_rays_train_backward_ex(capi.ptr(g_ws), g_img.data_ptr(), sigmas.data_ptr(), rgbs.data_ptr(), deltas.data_ptr(),
                                                                 rays.data_ptr(), ws.data_ptr(), image.data_ptr(), C.M, N, C.T_THRESH, gs.data_ptr(),
                                                                 gc.data_ptr(), bg_mode, 0.0, capi.ptr(bg), rows_used.data_ptr() if filled else None, st))
        got[filled] = (gs, gc)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    dead = torch.from_numpy(_dead_rows(early)).cuda()
    assert bool((got[True][0][dead] == 0).all()) and bool((got[True][1][dead] == 0).all()) and bool(torch.isfinite(got[True][0]).all())


# ------------------------------------------------------------------------------------------------
# 4. the gradient of depth
# ------------------------------------------------------------------------------------------------
def test_depth_has_a_gradient_and_composite_rays_train_still_has_none():
    import raymarching
    t, N = C.ray_table(False), len(C.RAYS)
    only_depth = dict(weights_sum=np.zeros(N), depth=np.ones(N), image=np.zeros((N, 3)), distortion=np.zeros(N))   # loss = depth.sum()
    ref = C.reference(t['sigmas'], t['rgbs'], t['deltas'], t['rays'], only_depth)
    f32 = C.prefix_form(t['sigmas'], t['rgbs'], t['deltas'], t['rays'], only_depth, torch.float32)
    got = _np(_run(raymarching.composite_rays_train_geo, False, torch.float32, {'depth': only_depth['depth']}))
    assert np.abs(got['grad_sigmas']).max() > 1e-3
    bound = 4.0 * float(np.abs(f32['grad_sigmas'] - ref['grad_sigmas']).max()) + 1e-7 * float(np.abs(ref['grad_sigmas']).max())
    err = float(np.abs(got['grad_sigmas'] - ref['grad_sigmas']).max())
    print(f'd depth / d sigmas: kernel error {err:.3e}, bound {bound:.3e}')
    assert err <= bound, (err, bound)
    assert (got['grad_rgbs'] == 0).all()
    # the reference op drops grad_depth (raymarching.py:275): unchanged
    old = _run(raymarching.composite_rays_train, False, torch.float32, {'depth': only_depth['depth']}, keys=KEYS[:3])
    assert (old['grad_sigmas'] == 0).all() and (old['grad_rgbs'] == 0).all()


def test_second_order_raises():
    import raymarching
    s, c, d, r = _inputs(False, torch.float32)
    depth = raymarching.composite_rays_train_geo(s, c, d, r, C.T_THRESH)[1]
    with pytest.raises(RuntimeError, match='second-order gradients are not provided'):
        torch.autograd.grad((depth ** 2).sum(), s, create_graph=True)


# ------------------------------------------------------------------------------------------------
# 5. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_two_calls_give_the_same_bits(dtype):
    import raymarching
    a = _run(raymarching.composite_rays_train_geo, True, dtype, C.upstream())
    b = _run(raymarching.composite_rays_train_geo, True, dtype, C.upstream())
    for key in a:
        assert torch.equal(a[key], b[key]) and not torch.isnan(a[key]).any(), key


# ------------------------------------------------------------------------------------------------
# 6. the renderer
# ------------------------------------------------------------------------------------------------
def test_renderer_geo_outputs_and_gradients():
    import raymarching
    import synthetic_scene as sc
    from nerf.network_ff import NeRFNetwork
    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1).to(dev).train()
    with torch.no_grad():
        model.encoder.embeddings.uniform_(-0.5, 0.5)
        # a hand-set occupancy: the cube of cells [40, 88)^3 of the 128^3 grid (the grid is stored in Morton order)
        ax = torch.arange(40, 88, dtype=torch.int32, device=dev)
        cells = raymarching.morton3D(torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)).long()
        model.density_grid.zero_()
        model.density_grid[0, cells] = 20.0
        model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    N = 256
    o, d, gt = sc.training_batch(N, seed=3)
    o, d, gt = cu(o), cu(d), cu(gt)
    kw = dict(staged=False, bg_color=1, perturb=False, force_all_rays=True, dt_gamma=0, max_steps=1024, T_thresh=C.T_THRESH)

    with torch.autocast('cuda', dtype=torch.float16):
        out = model.render(o[None], d[None], geo=True, **kw)
        assert set(out) == {'weights_sum', 'depth', 'image', 'depth_raw', 'distortion'}
        assert out['depth_raw'].shape == (N,) and out['distortion'].shape == (N,) and out['depth'].shape == (1, N)
        loss = ((out['image'][0] - gt) ** 2).mean() + 0.01 * out['distortion'].mean() + out['depth_raw'].mean()
    assert torch.isfinite(loss) and torch.isfinite(out['distortion']).all()   # also for a ray that misses the box (near = far, no samples)
    loss.backward()
    g = model.encoder.embeddings.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0
    assert torch.isfinite(model.sigma_net.weights.grad).all() and torch.isfinite(model.color_net.weights.grad).all()

    # the same call's samples, marched and evaluated here with the same counter state and (zero) noise (grad mode on, as in the call above:
    # the training and the inference network kernels are different kernels)
    with torch.autocast('cuda', dtype=torch.float16):
        nears, fars = raymarching.near_far_from_aabb(o, d, model.aabb_train, model.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        xyzs, dirs, deltas, rays = raymarching.march_rays_train(o, d, model.bound, model.density_bitfield, model.cascade, model.grid_size, nears, fars,
                                                                counter, model.mean_count, False, 128, True, 0, 1024)
        sigmas, rgbs = model(xyzs, dirs)
        sigmas, rgbs = (model.density_scale * sigmas).float().detach(), rgbs.float().detach()
        assert int(counter[0]) > 20 * N   # the cube is hit: tens of samples per ray
        # geo=False: the keys and the bits of composite_rays_train + _finish (the only path before this op existed)
        plain = model.render(o[None], d[None], **kw)
        assert set(plain) == {'weights_sum', 'depth', 'image'}
        ws0, depth0, image0 = raymarching.composite_rays_train(sigmas, rgbs, deltas, rays, C.T_THRESH)
        image0, depth0 = model._finish(image0, depth0, ws0, 1, nears, fars, (1, N))
        # (bit patterns: the normalised depth of a ray that misses the box is 0 / 0 = NaN, today as before)
        for key, want in (('weights_sum', ws0), ('depth', depth0), ('image', image0)):
            assert _bits_equal(plain[key].detach(), want), key
            assert _bits_equal(out[key].detach(), want), key
    # depth_raw and distortion against the float64 definition on those samples
    np64 = lambda t: t.double().cpu().numpy()
    rays_np = rays.cpu().numpy()
    ref = C.reference(np64(sigmas), np64(rgbs), np64(deltas), rays_np)
    zero_up = dict(weights_sum=np.zeros(N), depth=np.zeros(N), image=np.zeros((N, 3)), distortion=np.zeros(N))
    f32 = C.prefix_form(np64(sigmas), np64(rgbs), np64(deltas), rays_np, zero_up, torch.float32)
    span = np64(fars - nears)
    for key, got in (('depth', np64(out['depth_raw'].detach())), ('distortion', np64(out['distortion'].detach()) * span)):
        bound = 4.0 * float(np.abs(f32[key] - ref[key]).max()) + 1e-7 * float(np.abs(ref[key]).max())
        err = float(np.abs(got - ref[key]).max())
        print(f'renderer {key}: kernel error {err:.3e}, bound {bound:.3e}, max {np.abs(ref[key]).max():.3e}')
        # (the division and re-multiplication by far - near round twice more: 2 ulp of the value on top)
        assert err <= bound + 2 * 2.0 ** -23 * float(np.abs(ref[key]).max()), (key, err, bound)
    assert float(np.abs(ref['distortion']).max()) > 1e-4
