"""GPU: camera-pose gradients through the training rays (csrc/ray_gradient.hip) against the float64 models of
tests/ray_gradient_cases.py -- the per-ray reduction (exact where the sums are exact, a rounding bound elsewhere, NaN-poisoned rows that no
ray owns), the recovered sample parameters, gradcheck in float64, ngp_grid_input_gradient bit for bit on the lattice and within a rounding
bound off it, the pose backward, and the fused and drop-in training renders end to end."""
import ctypes

import numpy as np
import pytest
import torch

import composite_geo_cases as cg
import grid_forward_cases as gfc
import ray_gradient_cases as rg
import synthetic_scene as sc

pytestmark = pytest.mark.gpu
U = rg.U


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the ray reduction
# ---------------------------------------------------------------------------------------------------------------------
def _ray_backward(c, with_dir, with_sh, dtype=torch.float32):
    from raymarching import backend as rb
    t = {k: _cu(c[k]) for k in ('g_x', 'g_dir', 'xyzs', 'ts', 'rays_d')}
    t = {k: v.to(dtype) for k, v in t.items()}
    rays = _cu(c['rays'])
    go = torch.full((rg.RAY_N, 3), float('nan'), device='cuda', dtype=dtype)
    gd = torch.full_like(go, float('nan'))
    rb.ray_points_backward(t['g_x'], t['g_dir'] if with_dir else None, _cu(c['g_sh']) if with_sh else None, t['xyzs'], t['ts'], t['rays_d'], rays,
                           rg.RAY_M, rg.RAY_N, rg.RAY_BOUND, go, gd)
    return go.cpu().numpy(), gd.cpu().numpy()


@pytest.mark.parametrize('with_dir,with_sh', [(False, False), (True, False), (True, True)], ids=['xyz', 'xyz+dir', 'xyz+dir+sh'])
def test_ray_reduction_against_the_float64_model(with_dir, with_sh):
    c = rg.ray_case()
    want_o, want_d, S, K = rg.ray_backward_model(c['g_x'], c['g_dir'] if with_dir else None, c['g_sh'] if with_sh else None, c['xyzs'], c['ts'],
                                                 c['rays_d'], c['rays'], rg.RAY_BOUND)
    go, gd = _ray_backward(c, with_dir, with_sh)
    assert np.isfinite(go).all() and np.isfinite(gd).all()       # the NaN rows that no ray owns were never read
    assert np.array_equal(go.astype(np.float64), want_o)          # every partial sum is exact: bit for bit
    # K - 1 additions plus at most 8 roundings per term (64 with the SH terms: the fp32 Jacobian of the basis and its 16 products)
    bound = (K[:, None] + (64 if with_sh else 8)) * U * S
    err = np.abs(gd.astype(np.float64) - want_d)
    print('grad_rays_d: max err / bound = %.3f' % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    empty = [int(n) for n, off, cnt in c['rays'] if cnt == 0 or off + cnt > rg.RAY_M]
    assert len(empty) == 2 and (go[empty] == 0).all() and (gd[empty] == 0).all()
    assert np.abs(gd).min(axis=1).max() > 0
    # the same bits from a second launch
    go2, gd2 = _ray_backward(c, with_dir, with_sh)
    assert np.array_equal(go, go2) and np.array_equal(gd, gd2)
    # another assignment of output rows: the permuted result
    c2 = rg.ray_case(1)
    po, pd = _ray_backward(c2, with_dir, with_sh)
    for k in range(rg.RAY_N):
        assert np.array_equal(po[rg.PERM2[k]], go[cg.PERM[k]]) and np.array_equal(pd[rg.PERM2[k]], gd[cg.PERM[k]])


def test_ray_reduction_float64_twin():
    c = rg.ray_case()
    want_o, want_d, S, _ = rg.ray_backward_model(c['g_x'], c['g_dir'], None, c['xyzs'], c['ts'], c['rays_d'], c['rays'], rg.RAY_BOUND)
    go, gd = _ray_backward(c, True, False, torch.float64)
    assert np.array_equal(go, want_o)
    assert (np.abs(gd - want_d) <= 400 * 2.0 ** -53 * S).all()


def test_sample_ts_on_the_ray_table():
    import raymarching
    c = rg.ray_case()
    ts = raymarching.sample_ts(_cu(c['xyzs']), _cu(c['rays_o']), _cu(c['rays_d']), _cu(c['rays']), rg.RAY_BOUND).cpu().numpy()
    want = rg.ts_model(c['xyzs'], c['rays_o'], c['rays_d'], c['rays'], rg.RAY_BOUND)
    assert np.isfinite(ts).all() and (ts[c['used']:] == 0).all()
    # the quotient is formed in double and rounded once
    assert (np.abs(ts.astype(np.float64) - want) <= U * np.abs(want) * (1 + 2.0 ** -20)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. sample_ts / ray_points forward on the marcher's output
# ---------------------------------------------------------------------------------------------------------------------
def _marched(n_rays=64, max_steps=32, seed=11):
    import raymarching
    o, d, _ = sc.training_batch(n_rays, seed=seed)
    rng = np.random.default_rng(seed)
    o = (o * 0.45 + rng.uniform(-0.05, 0.05, o.shape)).astype(np.float32)   # origins about 1.45 from the centre, one per ray
    ro, rd = _cu(o), _cu(d)
    bitfield = torch.full((128 ** 3 // 8,), 255, dtype=torch.uint8, device='cuda')
    aabb = torch.tensor([-1., -1, -1, 1, 1, 1], device='cuda')
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device='cuda')
    xyzs, dirs, deltas, rays = raymarching.march_rays_train(ro, rd, 1.0, bitfield, 1, 128, nears, fars, counter, -1, False, 128, True, 0, max_steps)
    return ro, rd, xyzs, dirs, deltas, rays, int(counter[0].item())


def test_recovered_ts_rebuild_the_marchers_points():
    import raymarching
    ro, rd, xyzs, dirs, deltas, rays, used = _marched()
    assert used > 64 * 8 and xyzs.shape[0] % 128 == 0
    ts = raymarching.sample_ts(xyzs, ro, rd, rays, 1.0)
    x2, d2 = raymarching.ray_points(ro, rd, ts, rays, 1.0)
    assert torch.equal(d2, dirs)
    r = rays.cpu().numpy()
    o, d, t = ro.cpu().numpy().astype(np.float64), rd.cpu().numpy().astype(np.float64), ts.cpu().numpy().astype(np.float64)
    x, xr = xyzs.cpu().numpy().astype(np.float64), x2.cpu().numpy().astype(np.float64)
    worst = 0.0
    for n, off, cnt in r:
        sl = slice(off, off + cnt)
        # at most 6 roundings in t, one fma
        bound = 8 * U * (np.abs(o[n])[None] + np.abs(t[sl, None] * d[n][None]))
        err = np.abs(xr[sl] - x[sl])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (n, float((err / bound).max()))
    print('rebuilt points: max err / bound = %.3f' % worst)
    assert (xr[used:] == 0).all() and (t[used:] == 0).all()
    # like=: the marcher's own tensors, the same storage values
    ro_g = ro.clone().requires_grad_()
    x3, d3 = raymarching.ray_points(ro_g, rd, ts, rays, 1.0, like=(xyzs, dirs))
    assert torch.equal(x3, xyzs) and torch.equal(d3, dirs) and x3.requires_grad and x3.data_ptr() == xyzs.data_ptr()
    x3.sum().backward()
    inside = (xyzs.abs() < 1.0).float()
    want = torch.zeros(64, 3, device='cuda')
    for n, off, c in r:
        want[n] = inside[off:off + c].sum(0)
    assert torch.equal(ro_g.grad, want)


def test_ray_points_refuses_second_order():
    import raymarching
    ro, rd, xyzs, dirs, deltas, rays, used = _marched(8, 8)
    ts = raymarching.sample_ts(xyzs, ro, rd, rays, 1.0)
    ro_g = ro.clone().requires_grad_()
    x, _ = raymarching.ray_points(ro_g, rd, ts, rays, 1.0)
    up = torch.ones_like(x).requires_grad_()
    with pytest.raises(RuntimeError, match='second-order'):
        torch.autograd.grad(x, ro_g, grad_outputs=up, create_graph=True)


# ---------------------------------------------------------------------------------------------------------------------
# 3. gradcheck in float64
# ---------------------------------------------------------------------------------------------------------------------
def _small_rays():
    """3 rays x <= 5 samples, no sample within 1e-3 of +-bound"""
    rng = np.random.default_rng(5)
    o = rng.uniform(-0.3, 0.3, (3, 3))
    d = rng.standard_normal((3, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.array([[2, 0, 5], [0, 5, 3], [1, 8, 4]], np.int32)
    ts = rng.uniform(0.05, 0.6, 128)
    ts[12:] = 0.0
    for n, off, cnt in rays:
        x = o[n] + ts[off:off + cnt, None] * d[n]
        assert np.abs(np.abs(x) - 1.0).min() > 1e-3 and np.abs(x).max() < 1.0
    return _cu(o), _cu(d), _cu(ts), _cu(rays)


def test_gradcheck_ray_points():
    import raymarching
    o, d, ts, rays = _small_rays()
    o.requires_grad_()
    d.requires_grad_()
    fn = lambda o, d: raymarching.ray_points(o, d, ts, rays, 1.0)
    assert fn(o, d)[0].dtype == torch.float64
    assert torch.autograd.gradcheck(fn, (o, d), nondet_tol=0.0)


def test_gradcheck_of_the_whole_chain():
    """ray_points -> fp64 GridEncoder (4 levels, H = 4, finest resolution 32, smoothstep) || fp64 SHEncoder -> a two-layer torch MLP ->
    composite_rays_train (fp64) -> sum, in rays_o and rays_d.  The grid encoder takes its points in fp32 whatever the table's dtype
    (gridencoder: 'Float for inputs'), so a central difference of step eps carries the rounding of the points, <= 2^-24 / eps = 6e-4 of the
    slope at eps = 1e-4; a step across a cell boundary of the C^1 encoding adds eps / 4 * the jump of the second derivative, < 1 % of the
    slope at the finest level: rtol = 1e-2, atol = 1e-3 of outputs of order 1."""
    import raymarching
    from gridencoder import GridEncoder
    from shencoder import SHEncoder
    torch.manual_seed(3)
    o, d, ts, rays = _small_rays()
    enc = GridEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=4, per_level_scale=2.0, log2_hashmap_size=12,
                      interpolation='smoothstep').cuda().double()
    with torch.no_grad():
        enc.embeddings.uniform_(-1, 1)
    sh = SHEncoder(input_dim=3, degree=4).cuda()
    w1 = torch.randn(8 + 16, 16, device='cuda', dtype=torch.float64) * 0.4
    w2 = torch.randn(16, 4, device='cuda', dtype=torch.float64) * 0.4
    deltas = torch.zeros(128, 2, device='cuda', dtype=torch.float64)
    deltas[:12] = 0.05

    def fn(o, d):
        x, dirs = raymarching.ray_points(o, d, ts, rays, 1.0)
        feat = torch.cat([enc(x.float(), bound=1.0).double(), sh(dirs).double()], -1)
        h = torch.tanh(feat @ w1) @ w2
        ws, _depth, img = raymarching.composite_rays_train(torch.nn.functional.softplus(h[:, 0]), torch.sigmoid(h[:, 1:]), deltas, rays, 1e-4)
        return (ws.sum() + img.sum()).reshape(1)

    o.requires_grad_()
    d.requires_grad_()
    assert fn(o, d).dtype == torch.float64
    assert torch.autograd.gradcheck(fn, (o, d), eps=1e-4, atol=1e-3, rtol=1e-2, nondet_tol=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. ngp_grid_input_gradient
# ---------------------------------------------------------------------------------------------------------------------
def _grid_input_gradient(g, x, table, offs, S, H, gridtype, align, interp, bound):
    import _ngp_capi as capi
    M, L = x.shape[0], len(offs) - 1
    gt, xt, tt, ot = _cu(np.asarray(g, np.float16)), _cu(np.asarray(x, np.float32)), _cu(np.asarray(table, np.float32)).half(), _cu(np.asarray(offs, np.int32))
    out = torch.full((M, 3), float('nan'), device='cuda')
    capi.check(capi.lib.ngp_grid_input_gradient(gt.data_ptr(), xt.data_ptr(), tt.data_ptr(), ot.data_ptr(), M, 3, 2, L, float(S), int(H), int(gridtype),
                                                int(bool(align)), int(interp), capi.NGP_F16, float(bound), out.data_ptr(), capi.stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize('fc', rg.GRID_EXACT, ids=gfc.case_id)
def test_grid_input_gradient_on_the_lattice_is_exact(fc):
    b = fc.base
    ref = rg.grid_exact_reference(fc)
    for B in (b.B,) + rg.GRID_EXACT_BS:
        idx = gfc.point_index(fc, B)
        got = _grid_input_gradient(ref['g'][:, idx], ref['x'][idx], ref['table'], ref['offs'], 0.0, b.H, b.gridtype, b.align, b.interp, fc.bound)
        want = ref['want'][idx]
        assert np.array_equal(got.astype(np.float64), want), (B, int((got.astype(np.float64) != want).sum()))
        assert (got[~ref['inside'][idx]] == 0).all()


@pytest.mark.parametrize('interp,bound', rg.OFF_MODES)
def test_grid_input_gradient_off_the_lattice(interp, bound):
    c = rg.grid_off_lattice(interp, bound)
    got = _grid_input_gradient(c['g'], c['x'], c['emb'], c['offs'], c['S'], rg.OFF_H, 0, False, interp, bound).astype(np.float64)
    # at most 14 roundings inside a term, 32 accumulation steps
    tol = 64 * U * c['S_abs']
    err = np.abs(got - c['want'])
    print('off the lattice: max err / bound = %.3f' % float((err[c['inside']] / tol[c['inside']]).max()))
    assert (err <= tol).all(), float((err[c['inside']] / tol[c['inside']]).max())
    assert (got[~c['inside']] == 0).all()
    got2 = _grid_input_gradient(c['g'], c['x'], c['emb'], c['offs'], c['S'], rg.OFF_H, 0, False, interp, bound).astype(np.float64)
    assert np.array_equal(got, got2)


@pytest.mark.parametrize('interp', [0, 1])
def test_grid_input_gradient_is_no_less_accurate_than_the_dy_dx_route(interp):
    """relative L2 error against the existing route (encoder forward with dy_dx + the input backward) run on an fp32 copy of the table: the new
    kernel's error must not exceed that of the existing fp16 dy_dx route (dy_dx and grad_inputs rounded to the table dtype)"""
    from gridencoder.backend import _backend as gb
    c = rg.grid_off_lattice(interp, 0.0)
    B, L = rg.OFF_B, rg.OFF_L
    x, offs = _cu(c['x']), _cu(c['offs'].astype(np.int32))
    res = {}
    for dtype in (torch.float32, torch.float16):
        emb = _cu(c['emb']).to(dtype)
        g = _cu(c['g']).to(dtype)
        out = torch.empty(L, B, 2, device='cuda', dtype=dtype)
        dy_dx = torch.empty(B, L * 3 * 2, device='cuda', dtype=dtype)
        gb.grid_encode_forward(x, emb, offs, out, B, 3, 2, L, c['S'], rg.OFF_H, dy_dx, 0, False, interp)
        g_emb = torch.zeros_like(emb)
        g_in = torch.zeros(B, 3, device='cuda', dtype=dtype)
        gb.grid_encode_backward(g, x, emb, offs, g_emb, B, 3, 2, L, c['S'], rg.OFF_H, dy_dx, g_in, 0, False, interp)
        res[dtype] = g_in.double().cpu().numpy()
    new = _grid_input_gradient(c['g'], c['x'], c['emb'], c['offs'], c['S'], rg.OFF_H, 0, False, interp, 0.0).astype(np.float64)
    ref = res[torch.float32]
    e_new = np.linalg.norm(new - ref) / np.linalg.norm(ref)
    e_old = np.linalg.norm(res[torch.float16] - ref) / np.linalg.norm(ref)
    print('relative L2 against the fp32 route: new kernel %.3e, fp16 dy_dx route %.3e' % (e_new, e_old))
    assert e_new <= e_old, (e_new, e_old)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
@pytest.mark.parametrize('interp', [0, 1])
def test_encoder_forward_with_dy_dx_has_the_bits_of_the_forward_without(interp, dtype):
    """points that require grad take the dy_dx kernel: its outputs must be those of the scheduled kernels bit for bit (off the lattice, dense
    and hashed levels), or a render's forward would change with the rays' requires_grad"""
    from gridencoder.backend import _backend as gb
    c = rg.grid_off_lattice(interp, 0.0)
    B, L = rg.OFF_B, rg.OFF_L
    x, offs, emb = _cu(c['x']), _cu(c['offs'].astype(np.int32)), _cu(c['emb']).to(dtype)
    outs = []
    for with_dy in (False, True):
        out = torch.full((L, B, 2), float('nan'), device='cuda', dtype=dtype)
        dy_dx = torch.empty(B, L * 3 * 2, device='cuda', dtype=dtype) if with_dy else None
        gb.grid_encode_forward(x, emb, offs, out, B, 3, 2, L, c['S'], rg.OFF_H, dy_dx, 0, False, interp)
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().sum()) > 0
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the pose backward
# ---------------------------------------------------------------------------------------------------------------------
def _pose_backward(case):
    import _ngp_capi as capi
    fx, fy, cx, cy = rg.POSE_INTRINSICS
    go, gd = _cu(case['grad_o']), _cu(case['grad_d'])
    inds = None if case['inds'] is None else _cu(case['inds'])
    stride = 0 if inds is None or inds.dim() == 1 else case['n']
    out = torch.full((rg.POSE_B, 4, 4), float('nan'), device='cuda')
    capi.check(capi.lib.ngp_rays_from_pixels_backward(go.data_ptr(), gd.data_ptr(), rg.POSE_B, fx, fy, cx, cy, rg.POSE_W, capi.ptr(inds), stride,
                                                      case['n'], out.data_ptr(), capi.stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize('N,kind', [(N, kind) for N in rg.POSE_NS for kind in ('shared', 'per_pose')] + [(rg.POSE_H * rg.POSE_W, 'none')])
def test_pose_backward_against_float64_autograd(N, kind):
    case = rg.pose_case(N, kind)
    want, S = rg.pose_backward_model(case)
    got = _pose_backward(case)
    assert np.array_equal(got[:, :3, 3].astype(np.float64), want[:, :3, 3])      # integer-valued upstream: exact
    assert (got[:, 3] == 0).all()
    err = np.abs(got[:, :3, :3].astype(np.float64) - want[:, :3, :3])
    assert (err <= (case['n'] + 16) * U * S).all(), float((err / ((case['n'] + 16) * U * S)).max())
    assert np.array_equal(got, _pose_backward(case))


def test_pose_rays_has_the_bits_of_get_rays_and_differentiates():
    from nerf.utils import get_rays, pose_rays
    case = rg.pose_case(65, 'per_pose')
    poses = _cu(case['poses'])
    torch.manual_seed(0)
    ref = get_rays(poses, rg.POSE_INTRINSICS, rg.POSE_H, rg.POSE_W, N=24)
    inds = ref['inds'].contiguous()
    p = poses.clone().requires_grad_()
    ro, rd = pose_rays(p, rg.POSE_INTRINSICS, rg.POSE_H, rg.POSE_W, inds)
    assert torch.equal(ro, ref['rays_o']) and torch.equal(rd, ref['rays_d'])
    full = get_rays(poses, rg.POSE_INTRINSICS, rg.POSE_H, rg.POSE_W)
    fo, fd = pose_rays(p, rg.POSE_INTRINSICS, rg.POSE_H, rg.POSE_W)
    assert torch.equal(fo, full['rays_o']) and torch.equal(fd, full['rays_d'])
    w = torch.randn_like(rd)
    ((rd * w).sum() + ro.sum()).backward()
    p64 = torch.tensor(case['poses'].astype(np.float64), requires_grad=True)
    o64, d64, _ = rg.rays_from_pixels_torch(p64, rg.POSE_INTRINSICS, rg.POSE_W, inds.cpu(), 24)
    ((d64 * w.double().cpu()).sum() + o64.sum()).backward()
    assert torch.allclose(p.grad.double().cpu(), p64.grad, rtol=0, atol=1e-4)
    assert (p.grad[:, 3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------------------------------------------------
N_RAYS, MAX_STEPS, SCALE = 256, 32, 65536.0
# the sample buffer's size estimate: the <= 8192 samples of the batch fit, and the buffer is large enough for the grid backward's record
# sort (>= 16384 rows), whose sums are exact -- the table gradient is then reproducible on both paths and can be compared bit for bit
MEAN_COUNT = 20000


@pytest.fixture(scope='module')
def scene():
    import raymarching
    from nerf.network_ff import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1).cuda()
    with torch.no_grad():
        model.encoder.embeddings.uniform_(-0.5, 0.5)
        model.density_grid.fill_(100.0)
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    model.mean_count = MEAN_COUNT
    model.encoder.deterministic = True
    model.train()
    o, d, gt = sc.training_batch(N_RAYS, seed=21)
    return model, _cu(o)[None], _cu(d)[None], _cu(gt)


def _render(model, ro, rd, gt, fused, ray_grads):
    model.fused = fused
    model.zero_grad(set_to_none=True)
    ro = ro.clone().requires_grad_(ray_grads)
    rd = rd.clone().requires_grad_(ray_grads)
    with torch.autocast('cuda', dtype=torch.float16):
        assert model._fused_render_ok(ro.view(-1, 3), rd.view(-1, 3), 1, False) == fused
        out = model.render(ro, rd, staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=MAX_STEPS, T_thresh=1e-4)
        loss = ((out['image'][0] - gt) ** 2).mean()
    (loss * SCALE).backward()
    params = [p.grad.clone() for p in (model.encoder.embeddings, model.sigma_net.weights, model.color_net.weights)]
    fwd = [out[k].detach().clone() for k in ('image', 'depth', 'weights_sum')]
    return fwd, params, (ro.grad, rd.grad)


@pytest.fixture(scope='module')
def renders(scene):
    import fused
    model, ro, rd, gt = scene
    res = {}
    for f in (True, False):
        for ray_grads in (False, True):
            res[(f, ray_grads)] = _render(model, ro, rd, gt, f, ray_grads)
    fused.USE_FUSED_MID = False     # the generic branch of _network_backward, without ray gradients
    try:
        res['generic'] = _render(model, ro, rd, gt, True, False)
    finally:
        fused.USE_FUSED_MID = True
    model.fused = True
    return res


@pytest.mark.parametrize('fused_path', [True, False], ids=['fused', 'drop-in'])
def test_forward_bits_do_not_change_with_ray_gradients(renders, fused_path):
    plain, with_grads = renders[(fused_path, False)], renders[(fused_path, True)]
    for a, b, name in zip(plain[0], with_grads[0], ('image', 'depth', 'weights_sum')):
        assert torch.equal(a, b), name
    assert float(plain[0][2].min()) > 0.0 and plain[2] == (None, None)


def test_parameter_gradient_bits(scene, renders):
    import _ngp_capi as capi
    enc = scene[0].encoder
    arr = capi.host_offsets(enc.offsets)
    capacity = MEAN_COUNT + (128 - MEAN_COUNT % 128)
    assert N_RAYS * MAX_STEPS <= MEAN_COUNT
    assert capi.lib.ngp_grid_backward_is_reproducible(ctypes.cast(arr, ctypes.c_void_p), capacity, 3, 2, int(enc.num_levels), float(np.log2(enc.per_level_scale)),
                                                      int(enc.base_resolution), 0, 0, capi.NGP_F16) == 1
    for a, b, name in zip(renders[(False, False)][1], renders[(False, True)][1], ('embeddings', 'sigma_net', 'color_net')):
        assert torch.equal(a, b), ('drop-in', name)
    for a, b, name in zip(renders['generic'][1], renders[(True, True)][1], ('embeddings', 'sigma_net', 'color_net')):
        assert torch.equal(a, b), ('fused', name)
        assert float(a.abs().sum()) > 0


def test_fused_ray_gradients_agree_with_the_drop_in_ones(renders):
    """a dropped term, a sign or permuted rays give a difference of order 1; the drop-in side's fp16 hand-offs (dy_dx and grad_inputs in the
    table dtype) about 2^-11 per term: the sanity bar is 2^-6"""
    for k, name in ((0, 'rays_o'), (1, 'rays_d')):
        f, m = renders[(True, True)][2][k].double(), renders[(False, True)][2][k].double()
        assert torch.isfinite(f).all() and torch.isfinite(m).all() and float(m.norm()) > 0
        rel = float((f - m).norm() / m.norm())
        print('%s: fused vs drop-in relative L2 = %.3e' % (name, rel))
        assert rel < 2.0 ** -6, (name, rel)


def test_color_net_input_gradient_columns_are_written():
    """columns 0..15 of the colour net's input gradient (dL/dSH4) are written by ngp_ffmlp_backward_ex, whatever the buffer held"""
    import _ngp_capi as capi
    M, nl = 256, 3
    g = torch.Generator(device='cuda').manual_seed(4)
    half = dict(device='cuda', dtype=torch.half)
    color_in = (torch.rand(M, 32, device='cuda', generator=g) - 0.5).half()
    wc = ((torch.rand(64 * (32 + 64 * (nl - 1) + 16), device='cuda', generator=g) * 2 - 1) * (3 / 64) ** 0.5).half()
    fb, out16 = torch.zeros(nl, M, 64, **half), torch.zeros(M, 16, **half)
    capi.check(capi.lib.ngp_ffmlp_forward_ex(color_in.data_ptr(), wc.data_ptr(), M, 32, 16, 64, nl, 0, 6, fb.data_ptr(), out16.data_ptr(), 0, capi.stream()))
    g_out = (torch.randn(M, 16, device='cuda', generator=g) * 0.05).half()
    res = []
    for fill in (float('nan'), 7.0):
        g_in, g_w, scratch = torch.full((M, 32), fill, **half), torch.zeros_like(wc), torch.zeros(nl, M, 64, **half)
        capi.check(capi.lib.ngp_ffmlp_backward_ex(g_out.data_ptr(), color_in.data_ptr(), wc.data_ptr(), fb.data_ptr(), M, 32, 16, 64, nl, 0, 6, 1,
                                                  scratch.data_ptr(), g_in.data_ptr(), g_w.data_ptr(), 0, capi.stream()))
        res.append(g_in)
    assert torch.isfinite(res[0][:, :16]).all() and torch.equal(res[0][:, :16], res[1][:, :16]) and float(res[0][:, :16].abs().sum()) > 0


def test_recompute_mode_refuses_ray_gradients(scene):
    import fused
    model, ro, rd, gt = scene
    fused.USE_RECOMPUTE = True
    try:
        with pytest.raises(RuntimeError, match='NGP_FUSED_RECOMPUTE'):
            _render(model, ro, rd, gt, True, True)
    finally:
        fused.USE_RECOMPUTE = False


def test_pose_chain(scene):
    from nerf.utils import pose_rays
    model, _, _, gt = scene
    model.fused = True
    rng = np.random.default_rng(8)
    pose = np.concatenate([sc.camera_pose(rng), [[0, 0, 0, 1]]], 0).astype(np.float32)[None]
    inds = _cu(rng.integers(0, sc.RES * sc.RES, N_RAYS).astype(np.int64))
    grads = []
    for _ in range(2):
        poses = _cu(pose).requires_grad_()
        ro, rd = pose_rays(poses, (sc.FOCAL, sc.FOCAL, sc.RES / 2, sc.RES / 2), sc.RES, sc.RES, inds)
        with torch.autocast('cuda', dtype=torch.float16):
            out = model.render(ro, rd, staged=False, bg_color=1, perturb=False, force_all_rays=False, dt_gamma=0, max_steps=MAX_STEPS, T_thresh=1e-4)
            loss = ((out['image'][0] - gt) ** 2).mean()
        (loss * SCALE).backward()
        grads.append(poses.grad.clone())
    g = grads[0]
    assert torch.isfinite(g).all() and float(g[0, :3].abs().min()) > 0 and (g[0, 3] == 0).all()
    assert torch.equal(grads[0], grads[1])
