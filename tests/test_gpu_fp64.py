"""GPU: the fp64 path (fp64.hip) -- grid encoder forward / backward / TV, SH encoder, compositors, near_far / sph / packbits -- against fp64
CPU restatements, torch.autograd.gradcheck of the autograd Functions, bit-reproducibility of the grid backward, and the dtype boundary."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import grid_ordered_cases as goc
import oracle
from grid_forward_cases import grid_reference as _grid_reference   # the float64 model of the forward: the fp16 / fp32 kernels are pinned to it too

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _grid_backend(kind):
    if kind == 'ctypes':
        from gridencoder.backend import _backend
        return _backend
    import _gridencoder
    return _gridencoder


def _offsets(D, L, H, pls, log2T, align=False):
    """level offsets WITHOUT the rounding to multiples of 8 (the reference's gradcheck recipe builds them that way)"""
    offs, total = [0], 0
    for lvl in range(L):
        side = int(math.ceil(H * pls ** lvl)) + (0 if align else 1)
        total += min(2 ** log2T, side ** D)
        offs.append(total)
    return np.array(offs, np.int32)


def _dyadic_points(B, D, rng):
    """k / 2^10 in [0, 1]: with per_level_scale 2 and base 16 every level scale is an integer and every position is exact in fp32"""
    x = (rng.integers(0, 1025, (B, D)) / 1024.0).astype(np.float32)
    x[0, 0] = -1.0 / 1024    # outside: zeros, no gradient
    x[1, D - 1] = 1.0 + 1.0 / 1024
    x[2] = 0.0
    x[3] = 1.0
    return x


def _table(n, C, rng):
    """1 + k * 2^-40: differences vanish if anything is rounded through fp32"""
    return 1.0 + rng.integers(0, 1 << 20, (n, C)).astype(np.float64) * 2.0 ** -40


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want)
    bound = rel * np.abs(want) + rel * 1e-2 * max(1.0, float(np.abs(want).max(initial=0.0)))   # (+ a floor for values near zero)
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), got[bad][:4], want[bad][:4])


# ------------------------------------------------------------------------------------------------
# grid encoder
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [2, 3, 4, 5])
@pytest.mark.parametrize('C', [1, 2, 4, 8])
def test_grid_forward_matches_fp64_restatement(D, C):
    rng = np.random.default_rng(100 * D + C)
    B, L, H, S = 96, 3, 16, 1.0   # per_level_scale 2: level scales 15, 31, 63
    backend = _grid_backend('ctypes')
    for gridtype in (0, 1):
        for align in (False, True):
            for interp in (0, 1):
                offs = _offsets(D, L, H, 2.0, 10, align)
                emb = _table(int(offs[-1]), C, rng)
                x = _dyadic_points(B, D, rng)
                want_out, want_dy, _, _ = _grid_reference(x, emb, offs, S, H, gridtype, align, interp)
                xt, et, ot = torch.from_numpy(x).cuda(), torch.from_numpy(emb).cuda(), torch.from_numpy(offs).cuda()
                for with_dy in (True, False):
                    out = torch.empty(L, B, C, device='cuda', dtype=F64)
                    dy = torch.empty(B, L * D * C, device='cuda', dtype=F64) if with_dy else None
                    backend.grid_encode_forward(xt, et, ot, out, B, D, C, L, S, H, dy, gridtype, align, interp)
                    _close(out.cpu().numpy(), want_out)
                    if with_dy:
                        _close(dy.cpu().numpy().reshape(B, L, D, C), want_dy)


@pytest.mark.parametrize('kind', ['ctypes', 'compiled'])
@pytest.mark.parametrize('D,C,gridtype,align,interp', [(3, 2, 0, False, 0), (2, 4, 1, True, 1), (5, 1, 0, False, 1), (4, 8, 1, False, 0)])
def test_grid_backward_matches_fp64_restatement(kind, D, C, gridtype, align, interp):
    rng = np.random.default_rng(7 * D + C)
    B, L, H, S = 200, 3, 16, 1.0
    offs = _offsets(D, L, H, 2.0, 9, align)
    emb = _table(int(offs[-1]), C, rng)
    x = _dyadic_points(B, D, rng)
    grad = rng.standard_normal((L, B, C))
    _, want_dy, levels, _ = _grid_reference(x, emb, offs, S, H, gridtype, align, interp)
    want_ge = np.zeros_like(emb)
    for l, (gidx, ws, inside) in enumerate(levels):
        contrib = ws.astype(np.float64)[:, :, None] * grad[l][:, None, :]       # [B, 2^D, C]
        contrib[~inside] = 0
        np.add.at(want_ge, gidx.reshape(-1), contrib.reshape(-1, C))
    want_gi = np.einsum('lbc,bldc->bd', grad, want_dy)

    backend = _grid_backend(kind)
    xt, et, ot = torch.from_numpy(x).cuda(), torch.from_numpy(emb).cuda(), torch.from_numpy(offs).cuda()
    out = torch.empty(L, B, C, device='cuda', dtype=F64)
    dy = torch.empty(B, L * D * C, device='cuda', dtype=F64)
    backend.grid_encode_forward(xt, et, ot, out, B, D, C, L, S, H, dy, gridtype, align, interp)
    ge = torch.zeros_like(et)
    gi = torch.zeros(B, D, device='cuda', dtype=F64)
    backend.grid_encode_backward(torch.from_numpy(grad).cuda(), xt, et, ot, ge, B, D, C, L, S, H, dy, gi, gridtype, align, interp)
    _close(ge.cpu().numpy(), want_ge)
    _close(gi.cpu().numpy(), want_gi)


def test_grid_backward_is_bit_reproducible():
    """2^16 points into one 2^8-entry hashed level: thousands of contributions per entry, summed in a fixed order"""
    torch.manual_seed(0)
    B, D, C, L, H, S = 1 << 16, 3, 2, 1, 16, 1.0
    x = torch.rand(B, D, device='cuda')
    offs = torch.tensor([0, 256], dtype=torch.int32, device='cuda')
    emb = torch.randn(256, C, device='cuda', dtype=F64)
    grad = torch.randn(L, B, C, device='cuda', dtype=F64)
    runs = []
    for kind in ('compiled', 'ctypes', 'compiled'):
        ge = torch.zeros_like(emb)
        _grid_backend(kind).grid_encode_backward(grad, x, emb, offs, ge, B, D, C, L, S, H, None, None, 0, False, 0)
        runs.append(ge)
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    # sanity: the total equals the fp64 sum of every contribution (weights of a point sum to 1)
    assert abs(runs[0].sum().item() - grad.sum().item()) < 1e-6 * grad.abs().sum().item()


def _fp64_run_sums(keys, contrib, init):
    """the fp64 table gradient of one level from its records (slot order): per entry the contributions in ascending slot order, added left to
    right in float64 from 0.0, the sum added once to the entry's initial value"""
    k, v = goc.sorted_records(np.asarray(keys, np.int64), np.asarray(contrib, np.float64))
    want = init.copy()
    n = int((k != goc.NONE).sum())
    starts = np.flatnonzero(np.r_[True, k[1:n] != k[:n - 1]]) if n else np.zeros(0, np.int64)
    zero = np.zeros((1, v.shape[1]))
    for a, b in zip(starts, np.r_[starts[1:], n]):
        want[k[a]] = init[k[a]] + np.cumsum(np.vstack([zero, v[a:b]]), axis=0)[-1]
    return want


@pytest.mark.parametrize('one_cell', [False, True], ids=['B1000', 'one_cell_4133'])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('name', goc.LATTICE_NAMES)
def test_grid_table_gradient_has_the_bits_of_the_slot_order_model(name, order, one_cell):
    """The fp64 table gradient, first and second order, bit for bit against a model of its order, on the lattice cases of the ordered scatter
    (tests/grid_ordered_cases.py): every contribution w_k g / a_k g of the lattice level is exactly representable, so fma(coeff, g, acc) is
    acc + contribution.  About 3 % of the points lie outside [0,1]^D.  The lattice levels have 64 to 2^17 entries: one, two and three 8-bit
    digits of the record sort."""
    from gridencoder import backend, grid
    case = goc.lattice_case(name, order, False, one_cell)
    tab, level, size = case['tab'], case['level'], case['size']
    L, B, C = case['g'].shape
    D = tab['D']
    rng = np.random.default_rng(4300 + order + 2 * int(one_cell))
    x = np.array(case['x'])
    out = rng.choice(B, B // 32, replace=False)
    x[out, rng.integers(0, D, len(out))] = np.where(rng.random(len(out)) < 0.5, np.float32(-2.0 ** -20), np.nextafter(np.float32(1), np.float32(2)))
    keys = goc.record_keys(tab, x, level)
    contrib = goc.contributions(tab, x, case['g'], level, order, case['u'])
    outside = (keys.reshape(B, -1) == goc.NONE).all(axis=1)
    assert goc.fits_fp32(contrib) and outside[out].all() and 0.03 * B <= outside.sum() <= len(out) + 1   # (+ the lattice inputs' own one)
    assert (keys.reshape(B, -1)[~outside] != goc.NONE).all()
    assert {1: size < 256, 2: 256 <= size < 65536, 3: 65536 <= size}[{'A3d': 1, 'A3h': 3}.get(name, 2)]

    n = int(tab['offs'][-1])
    init = rng.standard_normal((n, C))
    xt, ot = torch.from_numpy(x).cuda(), torch.from_numpy(np.array(tab['offs'])).cuda()
    gt = torch.from_numpy(case['g'].astype(np.float64)).cuda()
    ge = torch.from_numpy(init).cuda()
    E = torch.from_numpy(rng.standard_normal((n, C))).cuda()
    if order == 1:
        backend.grid_encode_backward(gt, xt, E, ot, ge, B, D, C, L, tab['S'], tab['H'], None, None, tab['gridtype'], tab['align'], tab['interp'])
    else:
        ut = torch.from_numpy(case['u'].astype(np.float64)).cuda()
        grid.grid_encode_backward_backward(gt, xt, E, ot, ut, None, ge, None, B, D, C, L, tab['S'], tab['H'], tab['gridtype'], tab['align'],
                                           tab['interp'])
    lo, hi = int(tab['offs'][level]), int(tab['offs'][level + 1])
    want = _fp64_run_sums(keys, contrib, init[lo:hi])
    assert torch.equal(ge[lo:hi].cpu(), torch.from_numpy(want))
    assert np.count_nonzero(want != init[lo:hi]) > 0


def _reference_recipe():
    """testing/test_hashgrid_grad.py of the reference: D=3, L=4, C=2, base resolution 4, log2T=8, offsets without the /8 rounding"""
    D, L, C, H, log2T = 3, 4, 2, 4, 8
    offs = torch.from_numpy(_offsets(D, L, H, 2.0, log2T)).cuda()
    torch.manual_seed(0)
    emb = (torch.rand(int(offs[-1]), C, device='cuda', dtype=F64) * 2 - 1).requires_grad_()
    x = torch.rand(8, D, device='cuda')
    return x, emb, offs


@pytest.mark.parametrize('gridtype,interp', [(0, 0), (1, 1)])
def test_gradcheck_grid_encode(gridtype, interp):
    from gridencoder.grid import grid_encode
    x, emb, offs = _reference_recipe()
    fn = lambda e: grid_encode(x, e, offs, 2.0, 4, False, gridtype, False, interp)
    assert torch.autograd.gradcheck(fn, (emb,), eps=1e-2, atol=1e-3, rtol=0.01, nondet_tol=0.0)
    assert torch.autograd.gradcheck(fn, (emb,), nondet_tol=0.0)


def test_gradcheck_grid_encoder_module_double():
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=4, log2_hashmap_size=8).cuda().double()
    assert enc.embeddings.dtype == F64 and enc.offsets.dtype == torch.int32
    with torch.no_grad():
        enc.embeddings.uniform_(-1, 1)
    x = torch.rand(8, 3, device='cuda') * 2 - 1
    fn = lambda e: torch.func.functional_call(enc, {'embeddings': e}, (x,))
    emb = enc.embeddings.detach().clone().requires_grad_()
    assert fn(emb).dtype == F64
    assert torch.autograd.gradcheck(fn, (emb,), nondet_tol=0.0)
    # the module's own backward and TV on a float64 table (TV draws its random points in the table's dtype)
    enc(x).sum().backward()
    assert enc.embeddings.grad.dtype == F64
    g0 = enc.embeddings.grad.clone()
    enc.grad_total_variation(1e-3, B=4096)
    assert enc.embeddings.grad.dtype == F64 and not torch.equal(enc.embeddings.grad, g0)


def test_grad_total_variation_fp64():
    rng = np.random.default_rng(3)
    D, C, L, H, S = 3, 2, 3, 16, 1.0
    offs = _offsets(D, L, H, 2.0, 10)
    emb = rng.standard_normal((int(offs[-1]), C))
    x = (rng.integers(0, 1025, (500, D)) / 1024.0)
    want = oracle.grid_grad_tv(x.astype(np.float32), emb.astype(np.float32), np.zeros(emb.shape, np.float32), offs, 1e-2, S, H)
    got = torch.zeros(emb.shape, device='cuda', dtype=F64)
    _grid_backend('compiled').grad_total_variation(torch.from_numpy(x).cuda(), torch.from_numpy(emb).cuda(), got, torch.from_numpy(offs).cuda(), 1e-2,
                                                   500, D, C, L, S, H, 0, False)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------------------------------
# SH encoder
# ------------------------------------------------------------------------------------------------
def _sh_basis_fp64(dirs):
    """the 64 polynomials of tools/gen_sh.py evaluated in double by sympy's lambdify, and their symbolic derivatives"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_sh
    import sympy as sp
    Y = gen_sh.basis()
    xs = (gen_sh.x, gen_sh.y, gen_sh.z)
    cols = lambda exprs: np.stack([np.broadcast_to(np.asarray(sp.lambdify(xs, e, 'numpy')(*dirs.T), np.float64), dirs.shape[:1]) for e in exprs], -1)
    return cols(Y), [cols([sp.diff(e, v) for e in Y]) for v in xs]


@pytest.mark.parametrize('kind', ['ctypes', 'compiled'])
def test_sh_forward_matches_double_basis(kind):
    rng = np.random.default_rng(5)
    dirs = rng.standard_normal((300, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    Y, dY = _sh_basis_fp64(dirs)
    if kind == 'ctypes':
        from shencoder.backend import _backend
    else:
        import _shencoder as _backend
    x = torch.from_numpy(dirs).cuda()
    for deg in range(1, 9):
        N = deg * deg
        out = torch.empty(300, N, device='cuda', dtype=F64)
        dy = torch.empty(300, 3 * N, device='cuda', dtype=F64)
        _backend.sh_encode_forward(x, out, 300, 3, deg, dy)
        _close(out.cpu().numpy(), Y[:, :N])
        dy = dy.cpu().numpy().reshape(300, 3, N)
        for v in range(3):
            _close(dy[:, v], dY[v][:, :N])


def test_gradcheck_sh_encoder():
    from shencoder.sphere_harmonics import sh_encode
    torch.manual_seed(1)
    x = torch.nn.functional.normalize(torch.randn(6, 3, device='cuda', dtype=F64), dim=1).requires_grad_()
    for deg in range(1, 9):
        assert torch.autograd.gradcheck(lambda v: sh_encode(v, deg, True), (x,), nondet_tol=0.0), deg


# ------------------------------------------------------------------------------------------------
# compositing
# ------------------------------------------------------------------------------------------------
def _ray_batch(rng, n_rays=24, early=True):
    counts = rng.integers(1, 150, n_rays)
    counts[0] = 0
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]])
    M = int(counts.sum())
    rays = np.stack([np.arange(n_rays), offsets, counts], 1).astype(np.int32)
    sigmas = rng.uniform(0.1, 2.0, M)
    if early:
        for n in (1, 3, 5):   # rays that terminate early (T < T_thresh well before their last sample)
            sigmas[offsets[n]:offsets[n] + counts[n]] = 200.0
    rgbs = rng.uniform(0, 1, (M, 3))
    deltas = np.stack([rng.uniform(0.005, 0.05, M), rng.uniform(0.005, 0.05, M)], 1)
    return sigmas, rgbs, deltas, rays


def _composite_train_np(sigmas, rgbs, deltas, rays, T_thresh, grad_ws=None, grad_img=None):
    N = rays.shape[0]
    ws, depth, img = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    for index, off, num in rays:
        T, t = 1.0, 0.0
        for s in range(off, off + num):
            alpha = 1.0 - math.exp(-sigmas[s] * deltas[s, 0])
            w = alpha * T
            img[index] += w * rgbs[s]
            t += deltas[s, 1]
            depth[index] += w * t
            ws[index] += w
            T *= 1.0 - alpha
            if T < T_thresh:
                break
    if grad_ws is None:
        return ws, depth, img
    gs, gr = np.zeros_like(sigmas), np.zeros_like(rgbs)
    for index, off, num in rays:
        T, acc = 1.0, np.zeros(3)
        for s in range(off, off + num):
            alpha = 1.0 - math.exp(-sigmas[s] * deltas[s, 0])
            w = alpha * T
            acc += w * rgbs[s]
            T *= 1.0 - alpha
            gr[s] = grad_img[index] * w
            gs[s] = deltas[s, 0] * (np.dot(grad_img[index], T * rgbs[s] - (img[index] - acc)) + grad_ws[index] * (1.0 - ws[index]))
            if T < T_thresh:
                break
    return gs, gr


@pytest.mark.parametrize('kind', ['ctypes', 'compiled'])
def test_composite_rays_train_matches_fp64_loop(kind):
    if kind == 'ctypes':
        from raymarching.backend import _backend
    else:
        import _raymarching as _backend
    rng = np.random.default_rng(11)
    sigmas, rgbs, deltas, rays = _ray_batch(rng)
    M, N, T_thresh = sigmas.shape[0], rays.shape[0], 1e-4
    ws0, depth0, img0 = _composite_train_np(sigmas, rgbs, deltas, rays, T_thresh)
    assert (ws0[[1, 3, 5]] > 1 - 1e-4).all()
    g_ws, g_img = rng.standard_normal(N), rng.standard_normal((N, 3))
    want_gs, want_gr = _composite_train_np(sigmas, rgbs, deltas, rays, T_thresh, g_ws, g_img)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st, rt, dt, ry = cu(sigmas), cu(rgbs), cu(deltas), cu(rays)
    ws, depth, img = torch.empty(N, device='cuda', dtype=F64), torch.empty(N, device='cuda', dtype=F64), torch.empty(N, 3, device='cuda', dtype=F64)
    _backend.composite_rays_train_forward(st, rt, dt, ry, M, N, T_thresh, ws, depth, img)
    _close(ws.cpu().numpy(), ws0)
    _close(depth.cpu().numpy(), depth0)
    _close(img.cpu().numpy(), img0)
    gs, gr = torch.zeros_like(st), torch.zeros_like(rt)
    _backend.composite_rays_train_backward(cu(g_ws), cu(g_img), st, rt, dt, ry, ws, img, M, N, T_thresh, gs, gr)
    _close(gs.cpu().numpy(), want_gs, rel=1e-11)
    _close(gr.cpu().numpy(), want_gr)


def test_gradcheck_composite_rays_train():
    import raymarching
    rng = np.random.default_rng(2)
    sigmas, rgbs, deltas, rays = _ray_batch(rng, n_rays=6, early=False)
    sigmas = sigmas * 0.05   # T stays far above T_thresh under gradcheck's perturbations
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st, rt = cu(sigmas).requires_grad_(), cu(rgbs).requires_grad_()
    dt, ry = cu(deltas), cu(rays)
    ws, _, _ = _composite_train_np(sigmas, rgbs, deltas, rays, 1e-4)
    assert ws.max() < 0.9

    def fn(s, r):
        w, _depth, img = raymarching.composite_rays_train(s, r, dt, ry, 1e-4)
        return w, img   # (the depth output has no gradient, as in the reference)
    assert torch.autograd.gradcheck(fn, (st, rt), nondet_tol=0.0)


@pytest.mark.parametrize('kind', ['ctypes', 'compiled'])
def test_composite_rays_matches_fp64_loop(kind):
    if kind == 'ctypes':
        from raymarching.backend import _backend
    else:
        import _raymarching as _backend
    rng = np.random.default_rng(4)
    n_rays, n_alive, n_step, T_thresh = 40, 30, 8, 1e-2
    rays_alive = rng.permutation(n_rays)[:n_alive].astype(np.int32)
    rays_t = rng.uniform(0, 1, n_rays)
    ws0 = rng.uniform(0, 0.5, n_rays)
    ws0[rays_alive[:4]] = 0.995   # these stop at once
    depth0, img0 = rng.uniform(0, 1, n_rays), rng.uniform(0, 1, (n_rays, 3))
    sigmas = rng.uniform(0, 20, n_alive * n_step)
    rgbs = rng.uniform(0, 1, (n_alive * n_step, 3))
    deltas = np.stack([rng.uniform(0.01, 0.1, n_alive * n_step), rng.uniform(0.01, 0.1, n_alive * n_step)], 1)
    deltas[5 * n_step + 3:6 * n_step] = 0   # ray 5 ran out of samples
    # fp64 restatement (raymarching.cu:819-905)
    alive, t, ws, depth, img = rays_alive.copy(), rays_t.copy(), ws0.copy(), depth0.copy(), img0.copy()
    for n in range(n_alive):
        index, step = rays_alive[n], 0
        while step < n_step:
            i = n * n_step + step
            if deltas[i, 0] == 0:
                break
            alpha = 1.0 - math.exp(-sigmas[i] * deltas[i, 0])
            T = 1.0 - ws[index]
            w = alpha * T
            ws[index] += w
            t[index] += deltas[i, 1]
            depth[index] += w * t[index]
            img[index] += w * rgbs[i]
            if T < T_thresh:
                break
            step += 1
        if step < n_step:
            alive[n] = -1
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ra, rt, gw, gd, gi = cu(rays_alive), cu(rays_t), cu(ws0), cu(depth0), cu(img0)
    t_before = rt.clone()
    _backend.composite_rays(n_alive, n_step, T_thresh, ra, rt, cu(sigmas), cu(rgbs), cu(deltas), gw, gd, gi)
    assert ra.cpu().numpy().tolist() == alive.tolist() and (alive == -1).sum() >= 5
    stopped = rays_alive[alive == -1]
    want_t = t.copy()
    want_t[stopped] = rays_t[stopped]   # a ray that stopped keeps its t
    assert torch.equal(rt[cu(stopped).long()], t_before[cu(stopped).long()])
    _close(rt.cpu().numpy(), want_t)
    _close(gw.cpu().numpy(), ws)
    _close(gd.cpu().numpy(), depth)
    _close(gi.cpu().numpy(), img)


# ------------------------------------------------------------------------------------------------
# near_far_from_aabb, sph_from_ray, packbits
# ------------------------------------------------------------------------------------------------
def test_ray_utilities_fp64():
    import raymarching
    from oracle import torch_cpu
    torch.manual_seed(3)
    o = torch.randn(500, 3, dtype=F64) * 2
    d = torch.nn.functional.normalize(torch.randn(500, 3, dtype=F64), dim=1)
    aabb = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], dtype=F64)
    nears, fars = raymarching.near_far_from_aabb(o.cuda(), d.cuda(), aabb.cuda(), 0.25)
    assert nears.dtype == F64 and fars.dtype == F64
    want_n, want_f = torch_cpu.near_far_from_aabb(o, d, aabb, 0.25)
    miss = want_n == torch.finfo(torch.float32).max
    assert 0 < int(miss.sum()) < 500
    assert (nears.cpu()[miss] == torch.finfo(F64).max).all() and (fars.cpu()[miss] == torch.finfo(F64).max).all()
    assert torch.equal(nears.cpu()[~miss], want_n[~miss]) and torch.equal(fars.cpu()[~miss], want_f[~miss])

    coords = raymarching.sph_from_ray(o.cuda(), d.cuda(), 4.0)
    assert coords.dtype == F64
    np.testing.assert_allclose(coords.cpu().numpy(), torch_cpu.sph_from_ray(o, d, 4.0).numpy(), rtol=1e-13, atol=1e-14)

    grid = torch.rand(1, 64 ** 3, dtype=F64)
    grid[0, ::7] = 0.5 + 2.0 ** -40   # above the threshold in fp64, not after a rounding to fp32
    grid[0, 3::7] = 0.5
    bits = raymarching.packbits(grid.cuda(), 0.5).cpu().numpy()
    want = np.packbits((grid.numpy().reshape(-1, 8) > 0.5).astype(np.uint8), axis=1, bitorder='little').reshape(-1)
    assert np.array_equal(bits, want)


# ------------------------------------------------------------------------------------------------
# dtype boundary
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ctypes', 'compiled'])
def test_mixed_float64_calls_raise_naming_the_tensor(kind):
    if kind == 'ctypes':
        from gridencoder.backend import _backend as g
        from shencoder.backend import _backend as sh
        from raymarching.backend import _backend as rm
    else:
        import _gridencoder as g, _shencoder as sh, _raymarching as rm  # noqa: E401
    x = torch.rand(16, 3, device='cuda')
    offs = torch.tensor([0, 64], dtype=torch.int32, device='cuda')
    emb = torch.rand(64, 2, device='cuda', dtype=F64)
    with pytest.raises(RuntimeError, match='outputs'):
        g.grid_encode_forward(x, emb, offs, torch.empty(1, 16, 2, device='cuda'), 16, 3, 2, 1, 1.0, 4, None, 0, False, 0)
    with pytest.raises(RuntimeError, match='grad_embeddings'):
        g.grid_encode_backward(torch.rand(1, 16, 2, device='cuda', dtype=F64), x, emb, offs, torch.zeros(64, 2, device='cuda'), 16, 3, 2, 1, 1.0, 4,
                               None, None, 0, False, 0)
    with pytest.raises(RuntimeError, match='Float for inputs'):   # the grid encoder's inputs stay fp32
        g.grid_encode_forward(x.double(), emb, offs, torch.empty(1, 16, 2, device='cuda', dtype=F64), 16, 3, 2, 1, 1.0, 4, None, 0, False, 0)
    with pytest.raises(RuntimeError, match='outputs'):
        sh.sh_encode_forward(x.double(), torch.empty(16, 4, device='cuda'), 16, 3, 2, None)
    n = torch.empty(16, device='cuda', dtype=F64)
    with pytest.raises(RuntimeError, match='fars'):
        rm.near_far_from_aabb(x.double(), x.double(), torch.ones(6, device='cuda', dtype=F64), 16, 0.2, n, torch.empty(16, device='cuda'))
    rays = torch.zeros(4, 3, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='rgbs'):
        rm.composite_rays_train_forward(n, torch.rand(16, 3, device='cuda'), torch.rand(16, 2, device='cuda', dtype=F64), rays, 16, 4, 1e-4,
                                        n[:4].clone(), n[:4].clone(), torch.empty(4, 3, device='cuda', dtype=F64))


def test_march_rays_train_still_refuses_float64():
    import raymarching
    o = torch.rand(8, 3, device='cuda', dtype=F64)
    grid = torch.zeros(128 ** 3 // 8, dtype=torch.uint8, device='cuda')
    n, f = torch.zeros(8, device='cuda', dtype=F64), torch.ones(8, device='cuda', dtype=F64)
    with pytest.raises(RuntimeError, match='float32'):
        raymarching.march_rays_train(o, o, 1.0, grid, 1, 128, n, f)
