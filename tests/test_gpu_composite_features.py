"""GPU checks of the feature compositor raymarching.composite_rays_train_features (k_composite_feat_fwd / _bwd and their fp64 twins;
DESIGN.md 3.11) on the shared cases of tests/composite_features_cases.py: fp64 against the per-ray definition and autograd (+ gradcheck);
fp32 inside a yardstick measured from the float32 rounding of the same formulas on the CPU; rows no ray composites; consistency with
composite_rays_train; fp16 features with the bits of the fp32 op on the up-cast values; determinism; first order only; the renderer's
`aux`; normals out of a create_graph gradient, end to end in fp64.

Figures measured on MI355X (kernel error against the float64 definition, the CPU float32 error of the same formulas, bound = 4 x that + 1e-7
max|ref|) are in the docstrings below and in DESIGN.md 3.11.  The whole file takes about 9 s, 6 s of it the gradcheck."""
import numpy as np
import pytest
import torch

import composite_features_cases as F

pytestmark = pytest.mark.gpu


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _inputs(early, C, dtype, feat_dtype=None):
    t = F.ray_table(early)
    return (cu(t['sigmas'], dtype).requires_grad_(), cu(F.feats(C), feat_dtype or dtype).requires_grad_(), cu(t['deltas'], dtype), cu(t['rays']))


def _run(early, C, dtype, feat_dtype=None, backward=True):
    """forward (+ backward with upstream(C)) of the op -> dict of tensors (F.KEYS)"""
    import raymarching
    s, f, d, r = _inputs(early, C, dtype, feat_dtype)
    out = raymarching.composite_rays_train_features(s, f, d, r, F.T_THRESH)
    res = {'out': out.detach()}
    if backward:
        (cu(F.upstream(C), out.dtype) * out).sum().backward()
        res['grad_sigmas'], res['grad_feats'] = s.grad, f.grad
    return res


def _np(res):
    return {k: v.double().cpu().numpy() for k, v in res.items()}


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    view = torch.int16 if a.dtype == torch.float16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def _close(got, want, rel=1e-12):
    """the tolerance of tests/test_gpu_fp64.py::_close"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want)
    bound = rel * np.abs(want) + rel * 1e-2 * max(1.0, float(np.abs(want).max(initial=0.0)))
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), got[bad][:4], want[bad][:4])


# ------------------------------------------------------------------------------------------------
# 1. fp64 against the definition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('early', [True, False])
def test_fp64_forward_and_backward_match_the_definition(early):
    dead = F.dead_rows(early)
    for C in F.CHANNELS:
        ref, got = F.definition(early, C), _run(early, C, torch.float64)
        assert all(v.dtype == torch.float64 for v in got.values())
        got = _np(got)
        for key in F.KEYS:
            _close(got[key], ref[key])
        assert (got['grad_sigmas'][dead] == 0).all() and (got['grad_feats'][dead] == 0).all()


def test_fp64_gradcheck():
    import raymarching
    s, f, d, r = _inputs(False, 5, torch.float64)
    assert torch.autograd.gradcheck(lambda s_, f_: raymarching.composite_rays_train_features(s_, f_, d, r, F.T_THRESH), (s, f), nondet_tol=0.0)


# ------------------------------------------------------------------------------------------------
# 2. fp32 inside the float32 yardstick
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('early', [True, False])
def test_fp32_within_the_float32_yardstick(early):
    """out on both tables, the two gradients on the mild one (no sample on the T_thresh discontinuity).
    Measured on MI355X, smallest .. largest over the channel counts (kernel error / CPU float32 error / bound):
      out, early=True      7.7e-08 .. 3.5e-07 / 9.0e-08 .. 3.4e-07 / 3.9e-07 .. 1.5e-06
      out, early=False     1.8e-07 .. 3.5e-07 / 1.7e-07 .. 3.4e-07 / 6.8e-07 .. 1.5e-06
      grad_sigmas          9.6e-09 .. 1.4e-07 / 4.9e-09 .. 6.4e-08 / 2.2e-08 .. 2.8e-07   (closest: C = 130, 1.373e-07 against 2.516e-07)
      grad_feats           2.5e-08 .. 6.7e-08 / 2.6e-08 .. 7.7e-08 / 1.6e-07 .. 3.9e-07"""
    for C in F.CHANNELS:
        ref = F.definition(early, C)
        got = _run(early, C, torch.float32, backward=not early)
        assert all(v.dtype == torch.float32 for v in got.values())
        got = _np(got)
        for key in got:
            bound, cpu_err = F.yardstick(early, C, key)
            err = float(np.abs(got[key] - ref[key]).max())
            print(f'early={early} C={C} {key}: kernel error {err:.3e}, CPU float32 error {cpu_err:.3e}, bound {bound:.3e}')
            assert err <= bound, (C, key, err, bound)
        for name in ('empty', 'overflow'):
            assert (got['out'][F.PERM[[n for n, _ in F.RAYS].index(name)]] == 0).all()


# ------------------------------------------------------------------------------------------------
# 3. rows no ray composites
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feat_dtype', [torch.float32, torch.float16])
def test_backward_leaves_uncomposited_rows_exactly_zero(feat_dtype):
    dead = F.dead_rows(True)
    assert dead.sum() > 600   # behind the two early stops, the overflowing ray's rows, the padding
    for C in F.CHANNELS:
        got = _np(_run(True, C, torch.float32, feat_dtype))
        assert (got['grad_sigmas'][dead] == 0).all() and (got['grad_feats'][dead] == 0).all(), C
        assert (got['grad_sigmas'][~dead] != 0).all(), C


# ------------------------------------------------------------------------------------------------
# 4. consistency with composite_rays_train
# ------------------------------------------------------------------------------------------------
def test_consistent_with_composite_rays_train():
    """Measured on MI355X (distance from composite_rays_train / bound): image 5.960e-08 / 3.904e-07, weights_sum 5.960e-08 / 4.576e-07, depth
    1.192e-07 / 5.856e-07."""
    import raymarching
    import composite_geo_cases as G
    t = F.ray_table(True)
    s, d, r = cu(t['sigmas'], torch.float32), cu(t['deltas'], torch.float32), cu(t['rays'])
    rgbs = cu(t['rgbs'], torch.float32)
    ws, depth, image = raymarching.composite_rays_train(s, rgbs, d, r, F.T_THRESH)
    # the cumulative deltas[:, 1] along each ray: the t the compositors scan
    tt = np.zeros(F.M)
    for _, off, num in t['rays']:
        if num and off + num <= F.M:
            tt[off:off + num] = np.cumsum(t['deltas'][off:off + num, 1])
    chans = torch.cat([rgbs, torch.ones(F.M, 1, device='cuda'), cu(tt, torch.float32)[:, None]], 1)   # C = 5
    out = raymarching.composite_rays_train_features(s, chans, d, r, F.T_THRESH)
    for key, got, want in (('image', out[:, :3], image), ('weights_sum', out[:, 3], ws), ('depth', out[:, 4], depth)):
        bound, _ = G.yardstick(True, key)
        err = float((got.double() - want.double()).abs().max())
        print(f'{key}: against composite_rays_train {err:.3e}, bound {bound:.3e}')
        assert err <= bound, (key, err, bound)
        assert float(want.abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------
# 5. fp16 features
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [3, 22, 65])
def test_fp16_features_have_the_bits_of_the_fp32_op_on_the_upcast_values(C):
    for early in (True, False):
        half = _run(early, C, torch.float32, torch.float16)
        full = _run(early, C, torch.float32, torch.float32)   # feats(C) holds float16-representable values: the up-cast ones
        assert half['out'].dtype == torch.float32 and half['grad_sigmas'].dtype == torch.float32 and half['grad_feats'].dtype == torch.float16
        assert _bits_equal(half['out'], full['out']) and _bits_equal(half['grad_sigmas'], full['grad_sigmas'])
        assert _bits_equal(half['grad_feats'], full['grad_feats'].half())
        assert float(half['grad_feats'].float().abs().max()) > 1e-3


def test_autocast_does_not_upcast_fp16_features():
    import raymarching
    s, f, d, r = _inputs(True, 22, torch.float32, torch.float16)
    with torch.autocast('cuda', dtype=torch.float16):
        out = raymarching.composite_rays_train_features(s, f, d, r, F.T_THRESH)
    assert out.dtype == torch.float32 and _bits_equal(out.detach(), _run(True, 22, torch.float32, torch.float16, backward=False)['out'])
    out.sum().backward()
    assert f.grad.dtype == torch.float16 and s.grad.dtype == torch.float32


# ------------------------------------------------------------------------------------------------
# 6. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feat_dtype', [torch.float32, torch.float16])
def test_two_calls_give_the_same_bits(feat_dtype):
    for C in F.CHANNELS:
        a, b = _run(True, C, torch.float32, feat_dtype), _run(True, C, torch.float32, feat_dtype)
        for key in a:
            assert torch.equal(a[key], b[key]) and not torch.isnan(a[key].float()).any(), (C, key)


# ------------------------------------------------------------------------------------------------
# 7. first order only
# ------------------------------------------------------------------------------------------------
def test_second_order_raises():
    import raymarching
    s, f, d, r = _inputs(False, 5, torch.float32)
    out = raymarching.composite_rays_train_features(s, f, d, r, F.T_THRESH)
    with pytest.raises(RuntimeError, match='second-order gradients are not provided'):
        torch.autograd.grad((out ** 2).sum(), s, create_graph=True)


def test_channel_count_limits_and_empty_inputs():
    import raymarching
    t = F.ray_table(False)
    s, d, r = cu(t['sigmas'], torch.float32), cu(t['deltas'], torch.float32), cu(t['rays'])
    out = raymarching.composite_rays_train_features(s, torch.ones(F.M, 256, device='cuda'), d, r, F.T_THRESH)   # the largest C: four full blocks
    ws = raymarching.composite_rays_train(s, torch.zeros(F.M, 3, device='cuda'), d, r, F.T_THRESH)[0]
    assert out.shape == (F.N, 256) and torch.equal(out, out[:, :1].expand(-1, 256))
    # a ones channel gives weights_sum: two fp32 sums of K <= 300 non-negative terms with total <= 1, K 2^-24 each to first order
    assert float((out[:, 0] - ws).abs().max()) <= 2 * 300 * 2.0 ** -24 and float(ws.max()) > 0.5
    for C in (0, 257):
        with pytest.raises(RuntimeError, match=f'composite_rays_train_features_forward: C = {C}'):
            raymarching.composite_rays_train_features(s, torch.ones(F.M, C, device='cuda'), d, r, F.T_THRESH)
    none = raymarching.composite_rays_train_features(s[:0], torch.ones(0, 4, device='cuda'), d[:0], r[:1] * 0, F.T_THRESH)
    assert none.shape == (1, 4) and (none == 0).all()


# ------------------------------------------------------------------------------------------------
# 8. the renderer
# ------------------------------------------------------------------------------------------------
def test_renderer_aux():
    """Measured on MI355X: aux = rgbs is 2.980e-08 from image, bound 2 K 2^-24 = 3.242e-05 with K = 272."""
    import raymarching
    import synthetic_scene as sc
    from graph import GraphedTrainStep
    from nerf.network_ff import NeRFNetwork
    from optim import NGPAdam
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
    N = 128
    o, d, _ = sc.training_batch(N, seed=3)
    o, d = cu(o), cu(d)
    model.mean_count = 128 * N   # a sample estimate: the fused render is eligible (no host read-back)
    kw = dict(staged=False, bg_color=0, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=1024, T_thresh=F.T_THRESH)
    colour = lambda xyzs, dirs, sigmas, rgbs: rgbs
    with torch.autocast('cuda', dtype=torch.float16):
        assert model._fused_render_ok(o, d, 0, False) and not model._fused_render_ok(o, d, 0, False, aux=colour)
        out = model.render(o[None], d[None], aux=colour, **kw)
        assert set(out) == {'weights_sum', 'depth', 'image', 'aux'} and out['aux'].shape == (N, 3) and out['aux'].dtype == torch.float32
        # the autograd path without aux
        model.fused = False
        plain = model.render(o[None], d[None], **kw)
        model.fused = True
        assert set(plain) == {'weights_sum', 'depth', 'image'}
        for key in plain:   # (bit patterns: the normalised depth of a ray that misses the box is 0 / 0 = NaN)
            assert _bits_equal(out[key].detach().float(), plain[key].detach().float()), key
        # K: the largest sample count of a ray of this batch (the same march, zero noise)
        nears, fars = raymarching.near_far_from_aabb(o, d, model.aabb_train, model.min_near)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        rays = raymarching.march_rays_train(o, d, model.bound, model.density_bitfield, model.cascade, model.grid_size, nears, fars, counter,
                                            model.mean_count, False, 128, False, 0, 1024)[3]
    K = int(rays[:, 2].max())
    assert 20 < K <= 1024 and int(counter[0]) > 20 * N
    # bg_color = 0: image is the raw composite of rgbs.  Each kernel sums K non-negative fp32 terms with total <= 1: K 2^-24 each to first order
    err = float((out['aux'].detach().double() - out['image'][0].detach().double()).abs().max())
    print(f'renderer aux = rgbs against image: {err:.3e}, bound {2 * K * 2.0 ** -24:.3e} (K = {K})')
    assert err <= 2 * K * 2.0 ** -24 and float(out['image'].detach().abs().max()) > 0.1
    # a loss on aux alone trains the table and both MLPs
    model.zero_grad(set_to_none=True)
    (out['aux'] ** 2).mean().backward()
    for g in (model.encoder.embeddings.grad, model.sigma_net.weights.grad, model.color_net.weights.grad):
        assert g is not None and torch.isfinite(g).all() and float(g.float().abs().sum()) > 0
    # the graphed step keeps the autograd path
    opt = NGPAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    assert GraphedTrainStep(model, opt, None, N, kw)._direct_ok()
    assert not GraphedTrainStep(model, opt, None, N, dict(kw, aux=colour))._direct_ok()
    # eval mode
    with pytest.raises(NotImplementedError, match='aux'):
        model.eval().render(o[None], d[None], aux=colour, **kw)


# ------------------------------------------------------------------------------------------------
# 9. normals out of a create_graph gradient, end to end in fp64
# ------------------------------------------------------------------------------------------------
def test_normals_flow_into_the_second_order_graph_fp64():
    """grad_feats of the compositor flows back into the graph of normals = d sigma / d x (create_graph=True) and from there into the table.
    The reference writes the compositing in plain float64 torch from the same weights, twice: as a dense [N,M] product and as a per-ray sum.
    The two differ by their summation order alone; their distance in units of _close's bound at its rel is the condition the plain-torch run
    itself shows.  (The encoder takes float32 points whatever the table's dtype, so the gradient that enters the second-order graph is rounded
    to float32 on the way in, in all three runs alike.)  Measured on MI355X: the two plain-torch runs give the same bits (condition 0, so the
    comparison is _close at its rel), and so does the kernel run (distance 0.000e+00, max |grad| > 1e-3)."""
    import raymarching
    from gridencoder import GridEncoder
    torch.manual_seed(5)
    enc = GridEncoder(input_dim=3, num_levels=2, level_dim=2, base_resolution=4, log2_hashmap_size=8).cuda().double()
    with torch.no_grad():
        enc.embeddings.uniform_(-1, 1)
    t = F.ray_table(False)
    s, d, r = cu(t['sigmas']), cu(t['deltas']), cu(t['rays'])
    x0 = cu(np.random.default_rng(77).uniform(-1, 1, (F.M, 3)), torch.float32)   # the encoders take float32 points
    # the weights of the live samples, from the definition's formulas
    dense = np.zeros((F.N, F.M))
    for (index, off, _), k in zip(t['rays'], F.table_live(False)):
        if k:
            alpha = 1.0 - np.exp(-t['sigmas'][off:off + k] * t['deltas'][off:off + k, 0])
            dense[index, off:off + k] = alpha * np.cumprod(np.concatenate([[1.0], 1.0 - alpha[:-1]]))
    dense = cu(dense)

    def table_grad(composite):
        enc.embeddings.grad = None
        x = x0.clone().requires_grad_()
        sigma = torch.nn.functional.softplus(enc(x).sum(-1))
        assert sigma.dtype == torch.float64
        normals = torch.autograd.grad(sigma.sum(), x, create_graph=True)[0].double()
        assert normals.requires_grad and normals.shape == (F.M, 3)
        (composite(normals) ** 2).sum().backward()
        return enc.embeddings.grad.detach().cpu().numpy().copy()

    def per_ray(normals):
        rows = [normals.new_zeros(3)] * F.N
        for (index, off, _), k in zip(t['rays'], F.table_live(False)):
            if k:
                rows[index] = (dense[index, off:off + k, None] * normals[off:off + k]).sum(0)
        return torch.stack(rows)

    want = table_grad(lambda n: dense @ n)
    again = table_grad(per_ray)
    got = table_grad(lambda n: raymarching.composite_rays_train_features(s, n, d, r, F.T_THRESH))
    assert np.abs(want).max() > 1e-3
    rel = 1e-12
    unit = rel * np.abs(want) + rel * 1e-2 * max(1.0, float(np.abs(want).max()))
    cond = float((np.abs(again - want) / unit).max())
    print(f'normals: plain torch against itself {np.abs(again - want).max():.3e} = {cond:.3e} of the bound; '
          f'kernel {np.abs(got - want).max():.3e} = {float((np.abs(got - want) / unit).max()):.3e} of the bound')
    _close(got, want, rel * max(1.0, cond))
