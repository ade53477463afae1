"""GPU checks of the fused training step with geometry losses (csrc/raymarching.hip k_composite_train_geo_loss_bwd behind
ngp_composite_train_geo_loss_backward, fused.fused_train_iteration(geo_loss=), graph.GraphedTrainStep(geo_loss=)).

The kernel is held bit for bit to the entries it joins, on the ray table of tests/composite_geo_cases.py (N = 10, M = 1600: empty; 1, 63, 64,
65, 130 and 300 samples; saturating inside the first row; T_thresh crossed at the row boundary; an overflowing ray; shuffled output rows):
with zero lambdas to ngp_composite_train_loss_backward, with non-zero ones to the chain geo forward -> mse loss + per-ray gradients in fp32
torch -> geo backward -> rgb backward.  The iteration is held to autograd (model.render(geo=True)) and the graph replay to the eager
iteration at the bars of tests/test_gpu_graph.py."""
import functools

import numpy as np
import pytest
import torch

import composite_geo_cases as C
import synthetic_scene as sc

pytestmark = pytest.mark.gpu

N = len(C.RAYS)
BG_SCALAR = 0.7
LAMBDA_DISTORTION, LAMBDA_DEPTH = 0.5, 0.25
TINY = float(np.finfo(np.float32).tiny)


@functools.lru_cache(maxsize=None)
def _inputs(early):
    """the shared ray table as float32 device tensors + seeded per-ray inputs (fars > nears for every ray, some depth weights 0)"""
    dev = torch.device('cuda')
    t = C.ray_table(early)
    rng = np.random.default_rng(31)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    nears = rng.uniform(0.1, 0.5, N)
    m = rng.uniform(0.5, 1.5, N)
    for name in ('empty', 'row', 'long'):
        m[C.PERM[C.NAMES.index(name)]] = 0.0
    return dict(sigma=f(t['sigmas']), rgb=f(t['rgbs']), deltas=f(t['deltas']), rays=torch.from_numpy(t['rays']).to(dev).contiguous(),
                used=t['used'], nears=f(nears), fars=f(nears + rng.uniform(1.0, 3.0, N)), target=f(rng.uniform(0, 1, (N, 3))),
                bg=f(rng.uniform(0, 1, (N, 3))), z=f(rng.uniform(0.0, 2.0, N)), m=f(m),
                live=C.live_counts(t['sigmas'], t['deltas'], t['rays']))


def _workspace(inp):
    import _ngp_capi as capi
    ws = torch.zeros(capi.lib.ngp_march_rays_train_workspace_bytes(N) // 4, dtype=torch.int32, device='cuda')   # the marcher's workspace, tickets at 0
    ws[0] = inp['used']
    return ws


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device='cuda', dtype=dtype)


def _tickets_are_back(ws, inp):
    torch.cuda.synchronize()
    assert int(ws[0]) == inp['used'] and int(ws[1]) == 0 and int(ws[2:].abs().sum()) == 0


def _geo_loss_backward(inp, bg_mode, scale, with_loss, lam_dist, lam_depth, z, m):
    """the entry under test into NaN-filled buffers -> dict of its outputs (loss: None when left to the carrying launch)"""
    import _ngp_capi as capi
    i = inp
    ws = _workspace(i)
    out = dict(weights_sum=_nan(N), image=_nan(N, 3), depth=_nan(N), depth_raw=_nan(N), distortion=_nan(N), loss=_nan(1), ray_err=_nan(N),
               grad_sigmas=_nan(C.M), grad_out16=_nan(C.M, 16, dtype=torch.half))
    o = out
    assert capi.lib.ngp_composite_train_geo_loss_backward(
        i['sigma'].data_ptr(), i['rgb'].data_ptr(), i['deltas'].data_ptr(), i['rays'].data_ptr(), C.M, N, C.T_THRESH, bg_mode, BG_SCALAR,
        i['bg'].data_ptr() if bg_mode == 2 else None, i['nears'].data_ptr(), i['fars'].data_ptr(), i['target'].data_ptr(), lam_dist, lam_depth,
        capi.ptr(z), capi.ptr(m), capi.ptr(scale), o['weights_sum'].data_ptr(), o['image'].data_ptr(), o['depth'].data_ptr(),
        o['depth_raw'].data_ptr(), o['distortion'].data_ptr(), o['loss'].data_ptr() if with_loss else None, o['ray_err'].data_ptr(),
        o['grad_sigmas'].data_ptr(), o['grad_out16'].data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), capi.stream()) == 0
    _tickets_are_back(ws, i)
    if not with_loss:
        assert bool(torch.isnan(o['loss']).all())      # untouched: the sum is the carrying launch's
        o['loss'] = None
    return out


def _plain_loss_backward(inp, bg_mode, scale, with_loss):
    import _ngp_capi as capi
    i = inp
    ws = _workspace(i)
    o = dict(weights_sum=_nan(N), image=_nan(N, 3), depth=_nan(N), loss=_nan(1), ray_err=_nan(N), grad_sigmas=_nan(C.M),
             grad_out16=_nan(C.M, 16, dtype=torch.half))
    assert capi.lib.ngp_composite_train_loss_backward(
        i['sigma'].data_ptr(), i['rgb'].data_ptr(), i['deltas'].data_ptr(), i['rays'].data_ptr(), C.M, N, C.T_THRESH, bg_mode, BG_SCALAR,
        i['bg'].data_ptr() if bg_mode == 2 else None, i['nears'].data_ptr(), i['fars'].data_ptr(), i['target'].data_ptr(), capi.ptr(scale),
        o['weights_sum'].data_ptr(), o['image'].data_ptr(), o['depth'].data_ptr(), o['loss'].data_ptr() if with_loss else None,
        o['ray_err'].data_ptr(), o['grad_sigmas'].data_ptr(), o['grad_out16'].data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
        capi.stream()) == 0
    _tickets_are_back(ws, i)
    if not with_loss:
        o['loss'] = None
    return o


def _geo_forward(inp):
    import _ngp_capi as capi
    i = inp
    o = dict(weights_sum=_nan(N), depth_raw=_nan(N), image_raw=_nan(N, 3), dist=_nan(N))
    assert capi.lib.ngp_composite_rays_train_geo_forward(i['sigma'].data_ptr(), i['rgb'].data_ptr(), i['deltas'].data_ptr(), i['rays'].data_ptr(), C.M,
                                                         N, C.T_THRESH, o['weights_sum'].data_ptr(), o['depth_raw'].data_ptr(),
                                                         o['image_raw'].data_ptr(), o['dist'].data_ptr(), capi.stream()) == 0
    return o


def _span(inp):
    return (inp['fars'] - inp['nears']).clamp_min(TINY)


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('with_loss', [True, False])
@pytest.mark.parametrize('bg_mode', [1, 2])
@pytest.mark.parametrize('early', [True, False])
def test_zero_lambdas_are_the_plain_kernel(early, bg_mode, with_loss, scaled):
    inp = _inputs(early)
    scale = torch.tensor([128.0], device='cuda') if scaled else None
    got = _geo_loss_backward(inp, bg_mode, scale, with_loss, 0.0, 0.0, None, None)
    ref = _plain_loss_backward(inp, bg_mode, scale, with_loss)
    for key in ('weights_sum', 'image', 'depth', 'ray_err', 'grad_sigmas', 'grad_out16'):
        assert torch.equal(got[key], ref[key]), key
    if with_loss:
        assert torch.equal(got['loss'], ref['loss'])
    fwd = _geo_forward(inp)
    assert torch.equal(got['depth_raw'], fwd['depth_raw'])
    assert torch.equal(got['distortion'], fwd['dist'] / _span(inp))
    assert float(got['distortion'].max()) > 0 and float(got['grad_sigmas'].abs().max()) > 0


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device='cuda')


def _chain(inp, bg_mode, scale, lam_dist, lam_depth):
    """geo forward -> finish, mse loss (ngp_pipeline_mse_loss) and the per-ray gradients gw, gd, gl in float32 torch, one torch op per
    operation the kernel writes -> geo backward into zeroed buffers -> rgb backward.  -> grad_sigmas, grad_out16, ray_err, per-ray terms"""
    import _ngp_capi as capi
    i = inp
    st = capi.stream()
    fwd = _geo_forward(i)
    bgv = i['bg'] if bg_mode == 2 else torch.full((N, 3), BG_SCALAR, device='cuda')
    image = fwd['image_raw'] + (1.0 - fwd['weights_sum'])[:, None] * bgv
    loss, gimg = _nan(1), _nan(N, 3)
    assert capi.lib.ngp_pipeline_mse_loss(image.data_ptr(), i['target'].data_ptr(), 3 * N, capi.ptr(scale), loss.data_ptr(), gimg.data_ptr(), st) == 0
    s = scale[0] if scale is not None else _f32(1.0)
    gw = torch.zeros(N, device='cuda') - ((gimg[:, 0] * bgv[:, 0] + gimg[:, 1] * bgv[:, 1]) + gimg[:, 2] * bgv[:, 2])
    span = _span(i)
    dn = fwd['dist'] / span
    gl = ((_f32(lam_dist) / _f32(float(N))) / span) * s
    dz = fwd['depth_raw'] - i['z']
    gd = ((((_f32(2.0) * _f32(lam_depth)) / _f32(float(N))) * i['m']) * dz) * s
    term = _f32(lam_dist) * dn + _f32(lam_depth) * (i['m'] * (dz * dz))      # per output row
    gs, grgb = torch.zeros(C.M, device='cuda'), torch.zeros(C.M, 3, device='cuda')
    assert capi.lib.ngp_composite_rays_train_geo_backward(gw.data_ptr(), gd.data_ptr(), gimg.data_ptr(), gl.data_ptr(), i['sigma'].data_ptr(),
                                                          i['rgb'].data_ptr(), i['deltas'].data_ptr(), i['rays'].data_ptr(),
                                                          fwd['weights_sum'].data_ptr(), fwd['depth_raw'].data_ptr(), fwd['image_raw'].data_ptr(),
                                                          fwd['dist'].data_ptr(), C.M, N, C.T_THRESH, gs.data_ptr(), grgb.data_ptr(), st) == 0
    g16 = _nan(C.M, 16, dtype=torch.half)
    assert capi.lib.ngp_pipeline_rgb_backward(grgb.data_ptr(), i['rgb'].data_ptr(), g16.data_ptr(), C.M, st) == 0
    # the per-ray squared error is the plain entry's (fma(e2, e2, fma(e1, e1, e0 e0)): no torch op rounds like it); + 3 x the ray's two terms
    err = _plain_loss_backward(i, bg_mode, scale, False)['ray_err'] + _f32(3.0) * term[i['rays'][:, 0].long()]
    torch.cuda.synchronize()
    return dict(grad_sigmas=gs, grad_out16=g16, ray_err=err, image=image, depth_raw=fwd['depth_raw'], distortion=dn)


def _live_mask(inp):
    mask = torch.zeros(C.M, dtype=torch.bool)
    for (_, off, _), k in zip(inp['rays'].tolist(), inp['live']):
        mask[off:off + k] = True
    return mask.cuda()


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('bg_mode', [1, 2])
@pytest.mark.parametrize('early', [True, False])
def test_nonzero_lambdas_are_the_chain_of_existing_entries(early, bg_mode, scaled):
    inp = _inputs(early)
    scale = torch.tensor([128.0], device='cuda') if scaled else None
    assert bool((inp['fars'] > inp['nears']).all()) and int((inp['m'] == 0).sum()) == 3
    ref = _chain(inp, bg_mode, scale, LAMBDA_DISTORTION, LAMBDA_DEPTH)
    # precondition, on the chain alone: each term moves grad_sigmas on more than half of the live rays by more than 2^-10 relative
    rays, live = inp['rays'].tolist(), inp['live']
    n_live = sum(1 for k in live if k)
    assert n_live == 8
    for name, lams in (('distortion', (0.0, LAMBDA_DEPTH)), ('depth', (LAMBDA_DISTORTION, 0.0))):
        without = _chain(inp, bg_mode, scale, *lams)['grad_sigmas']
        moved = 0
        for (_, off, _), k in zip(rays, live):
            if k:
                full = ref['grad_sigmas'][off:off + k]
                moved += float((full - without[off:off + k]).abs().max()) > 2.0 ** -10 * float(full.abs().max())
        print(f'{name} term moves grad_sigmas on {moved} of {n_live} live rays')
        assert moved > n_live // 2, (name, moved)
    got = _geo_loss_backward(inp, bg_mode, scale, True, LAMBDA_DISTORTION, LAMBDA_DEPTH, inp['z'], inp['m'])
    for key in ('grad_sigmas', 'grad_out16', 'ray_err', 'image', 'depth_raw', 'distortion'):
        assert torch.equal(got[key], ref[key]), (key, float((got[key].float() - ref[key].float()).abs().max()))
    # no NaN of the prefill survives, and every row the chain leaves at zero is zero: behind an early stop, the overflowing ray's, rows >= used
    assert bool(torch.isfinite(got['grad_sigmas']).all()) and bool(torch.isfinite(got['grad_out16'].float()).all())
    dead = ~_live_mask(inp)
    assert int(dead.sum()) >= C.M - inp['used'] + (300 if early else 0)
    assert bool((ref['grad_sigmas'][dead] == 0).all()) and bool((ref['grad_out16'][dead] == 0).all())
    assert bool((got['grad_sigmas'][dead] == 0).all()) and bool((got['grad_out16'][dead] == 0).all())
    assert bool((got['grad_out16'][:, 3:] == 0).all())
    # the loss VALUE: loss_sum_block adds N non-negative terms, each through at most ceil(N / 256) + 10 roundings: under 2^-20 relative
    want = float(ref['ray_err'].double().sum()) / (3 * N)
    print(f'loss {float(got["loss"])!r} against {want!r}')
    assert bool((ref['ray_err'] >= 0).all()) and abs(float(got['loss']) - want) <= 4e-6 * want
    # ... and left to the carrying launch, the per-ray terms are the same
    deferred = _geo_loss_backward(inp, bg_mode, scale, False, LAMBDA_DISTORTION, LAMBDA_DEPTH, inp['z'], inp['m'])
    assert torch.equal(deferred['ray_err'], got['ray_err']) and torch.equal(deferred['grad_sigmas'], got['grad_sigmas'])


def test_deterministic():
    inp = _inputs(True)
    scale = torch.tensor([128.0], device='cuda')
    a = _geo_loss_backward(inp, 2, scale, True, LAMBDA_DISTORTION, LAMBDA_DEPTH, inp['z'], inp['m'])
    b = _geo_loss_backward(inp, 2, scale, True, LAMBDA_DISTORTION, LAMBDA_DEPTH, inp['z'], inp['m'])
    for key in a:
        assert torch.equal(a[key].view(torch.int16 if a[key].dtype == torch.half else torch.int32),
                           b[key].view(torch.int16 if b[key].dtype == torch.half else torch.int32)), key


# ---------------------------------------------------------------------------------------------------------------------------------
# the iteration
# ---------------------------------------------------------------------------------------------------------------------------------
# lambda of the end-to-end tests: 4.  Two conditions set it.  (1) The gradient must show the term above the bars of the autograd comparison:
# the MSE gradient of a ray's weights is 2 e / 3N with |e| ~ 0.3, the distortion's lambda / (N span) times d dist / d w ~ the ray's extent
# in t over a span of ~2, so from lambda ~ 1 on the two are of one size (asserted on the autograd side, ten times each bar).  (2) The loss
# VALUE must show it above the bar of the graph-replay comparison, 8e-2 * 0.27 + 2e-3 = 0.024 at this scene's loss: the freshly initialised
# model's mean normalised distortion on these batches is 0.013 (read off the reference runs: the difference of the eager loss with and
# without the term at the first step, lambda = 1), so lambda must exceed 1.9; 4 leaves a factor two.  (mip-NeRF 360 trains with 0.01, where
# the term sits inside the noise these bars allow for and the tests would see nothing.)
LAMBDA_E2E = 4.0
KW = dict(staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4)


def _make_ngp(dev):
    import raymarching
    from nerf.network_ff import NeRFNetwork
    from optim import NGPAdam
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_thresh=10).to(dev)
    model.train()
    model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.iter_density = 16
    opt = NGPAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    return model, opt


def _batch(dev, n_rays, seed):
    o, d, gt = sc.training_batch(n_rays, seed=seed)
    return torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev), torch.from_numpy(gt).to(dev)


def test_iteration_with_geo_loss_matches_the_autograd_iteration():
    """fused.fused_train_iteration(geo_loss=GeoLoss(lambda_distortion)) against model.render(geo=True) -> mse + lambda * distortion.mean() ->
    scaled backward, at the shapes of tests/test_gpu_graph.py::test_autograd_free_iteration_matches_autograd_iteration (1024 rays,
    mean_count 60 * 1024) and at its bars.  The colour network's weight gradient cannot see the term (the distortion is a function of the
    densities alone; its gradient reaches the colour network's WEIGHTS through nothing), so the visibility precondition is asserted on the
    hash table and the density network and the colour weights are asserted to be indifferent to lambda on the autograd side."""
    from fused import GeoLoss, fused_train_iteration
    dev = torch.device('cuda')
    model, opt = _make_ngp(dev)
    n_rays = 1024
    o, d, gt = _batch(dev, n_rays, 5)
    model.mean_count = 60 * n_rays
    params = (model.encoder.embeddings, model.sigma_net.weights, model.color_net.weights)

    def autograd(lam):
        model.local_step = 0
        with torch.autocast('cuda', dtype=torch.float16):
            out = model.render(o, d, geo=True, **KW)
            loss = torch.nn.functional.mse_loss(out['image'][0], gt) + lam * out['distortion'].mean()
        opt.scale(loss).backward()
        grads = [p._ngp_grad16.clone() for p in params]
        assert all(p.grad is None for p in params)
        opt.flat_grad16.zero_()
        return out, loss, grads, model.step_counter[0].clone()

    _, _, grads_0, _ = autograd(0.0)
    out, loss_a, grads_a, count_a = autograd(LAMBDA_E2E)
    # the term is visible: with and without it the reference gradients differ by more than ten times each bar
    for name, ga, g0 in zip(('table', 'sigma net'), grads_a[:2], grads_0[:2]):
        ga, g0 = ga.float(), g0.float()
        d_max, d_mean = float((ga - g0).abs().max()), float((ga - g0).abs().mean())
        print(f'{name}: lambda moves the gradient by max {d_max:.3e} (max |g| {float(ga.abs().max()):.3e}), mean {d_mean:.3e} '
              f'(mean |g| {float(ga.abs().mean()):.3e})')
        assert d_max > 10 * 2e-2 * float(ga.abs().max()) and d_mean > 10 * 1e-3 * float(ga.abs().mean()), name
    assert torch.equal(grads_a[2], grads_0[2])     # the colour weights: indifferent to lambda
    assert float(out['distortion'].detach().max()) > 0

    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    capacity = model.mean_count + (128 - model.mean_count % 128)
    args = (model, o, d, gt, model.aabb_train, counter, capacity, opt.scalars[0:1], 1, False, 0, 1024, 1e-4)
    res = fused_train_iteration(*args, geo_loss=GeoLoss(lambda_distortion=LAMBDA_E2E))
    assert len(res) == 6
    loss_d, image, depth, ws, depth_raw, distortion = res
    grads_d = [p._ngp_grad16.clone() for p in params]
    opt.flat_grad16.zero_()
    assert torch.equal(counter, count_a)
    assert torch.equal(image, out['image'][0])
    assert torch.allclose(depth, out['depth'][0], rtol=0, atol=0, equal_nan=True)
    assert torch.equal(depth_raw, out['depth_raw']) and torch.equal(distortion, out['distortion'])
    print(f'loss {loss_d.item()!r} against autograd {loss_a.item()!r}')
    np.testing.assert_allclose(loss_d.item(), loss_a.item(), rtol=2e-6)
    for name, ga, gd in zip(('table', 'sigma net', 'colour net'), grads_a, grads_d):
        ga, gd = ga.float(), gd.float()
        d_max, d_mean = float((ga - gd).abs().max()), float((ga - gd).abs().mean())
        print(f'{name}: max |d| {d_max:.3e} of max |g| {float(ga.abs().max()):.3e}, mean |d| {d_mean:.3e} of mean |g| {float(ga.abs().mean()):.3e}')
        assert float(ga.abs().max()) > 0
        assert d_max <= 2e-2 * float(ga.abs().max()), name
        assert d_mean <= 1e-3 * float(ga.abs().mean()) + 1e-12, name

    # all lambdas zero: the gradients of the plain call, bit for bit
    def deposited(**kw):
        r = fused_train_iteration(*args, **kw)
        g = [p._ngp_grad16.clone() for p in params]
        opt.flat_grad16.zero_()
        return r, g

    r_plain, g_plain = deposited()
    r_zero, g_zero = deposited(geo_loss=GeoLoss())
    assert len(r_plain) == 4 and len(r_zero) == 6
    for a, b in zip(r_plain, r_zero[:4]):
        assert torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)     # (depth is 0 / 0 for a ray that misses the box, in both)
    for a, b in zip(g_plain, g_zero):
        assert torch.equal(a, b)


def test_graph_replay_with_geo_loss_matches_the_eager_iteration():
    """three steps of GraphedTrainStep(geo_loss=) (captured at once: the sample estimate is given; table Adam fused into the grid backward)
    against three eager fused_train_iteration(geo_loss=) + optimizer steps on a twin model, at the bars of
    tests/test_gpu_graph.py::test_graph_replay_matches_eager_iteration; the same three eager steps without the term end elsewhere."""
    from fused import GeoLoss, fused_train_iteration
    from graph import GraphedTrainStep
    dev = torch.device('cuda')
    n_rays = 1024
    batches = [_batch(dev, n_rays, 300 + i) for i in range(3)]
    geo = GeoLoss(lambda_distortion=LAMBDA_E2E)

    model, opt = _make_ngp(dev)
    model.mean_count = 60 * n_rays
    st = GraphedTrainStep(model, opt, None, n_rays, KW, direct=True, fused_table_adam=True, capacity_ladder=(), geo_loss=geo)
    st.global_step = 1            # no occupancy refresh inside the three steps (it would replace the given sample estimate)
    graphed = [float(st.step(*b)) for b in batches]
    assert st.capture_error is None and st.n_captures == 1 and st.used_direct and st.table_fused
    capacity = st.captured_capacity
    st.close()

    def eager(geo_loss):
        model, opt = _make_ngp(dev)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        losses = []
        for o, d, gt in batches:
            res = fused_train_iteration(model, o, d, gt, model.aabb_train, counter, capacity, opt.scalars[0:1], 1, False, 0, 1024, 1e-4,
                                        geo_loss=geo_loss)
            opt.step()
            losses.append(float(res[0]))
        return losses

    with_term, without = eager(geo), eager(None)
    print('graphed', graphed, 'eager', with_term, 'eager without the term', without)
    assert np.isfinite(graphed).all()
    np.testing.assert_allclose(graphed, with_term, rtol=8e-2, atol=2e-3)
    assert all(abs(a - b) > 8e-2 * abs(b) + 2e-3 for a, b in zip(graphed, without))
