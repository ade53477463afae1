"""GPU checks of raymarching.sdf_sigmas (k_sdf_sigmas_fwd / _bwd / _inv_s and their fp64 instances) on the shared table of
tests/sdf_sigmas_cases.py: fp32 forward and backward over the (inv_s, cos_anneal) grid inside a yardstick measured from the float32 rounding
of the same definition on the CPU; exact zeros on capped and padding rows; bit reproducibility, grad_inv_s included; every row count around
the wave and workgroup sizes as a bit-identical prefix of the full run; fp64 against the float64 definition (+ gradcheck); fp16 under
autocast; the optional dirs gradient; no second order; and the op composed with the training compositors against NeuS's own rendering.

Figures measured on MI355X: DESIGN.md 3.16."""
import numpy as np
import pytest
import torch

import composite_geo_cases as G
import sdf_sigmas_cases as C

pytestmark = pytest.mark.gpu

GRAD_KEYS = C.KEYS[1:]


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _bits_equal(a, b):
    a, b = a.contiguous(), b.contiguous()
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def _run(inv_s, cos_anneal, dtype, rows=C.M, dirs_grad=True, cast=None):
    """the op on the first `rows` rows of the table, backward with the table's upstream gradient -> dict of tensors: sigma, grad_*
    (grad_dirs None without dirs_grad); cast: the dtype the row tensors are handed over in (default: `dtype`)"""
    import raymarching
    t = C.sample_table()
    leaf = lambda k, grad=True: cu(t[k][:rows], dtype).to(cast or dtype).requires_grad_(grad)
    sdf, normals, dirs, deltas = leaf('sdf'), leaf('normals'), leaf('dirs', dirs_grad), leaf('deltas', False)
    s = torch.tensor([inv_s], dtype=dtype, device='cuda', requires_grad=True)
    sigma = raymarching.sdf_sigmas(sdf, normals, dirs, deltas, s, cos_anneal)
    sigma.backward(cu(t['up'][:rows], sigma.dtype))
    return dict(sigma=sigma.detach(), grad_sdf=sdf.grad, grad_normals=normals.grad, grad_dirs=dirs.grad, grad_inv_s=s.grad)


def _errors(res, ref, rows=C.M):
    """max |error| per key of C.KEYS against the float64 reference (x = sigma * d0)"""
    d0 = C.sample_table()['deltas'][:rows, 0]
    got = {k: res[k].double().cpu().numpy() for k in GRAD_KEYS}
    got['x'] = res['sigma'].double().cpu().numpy() * d0
    return {k: float(np.abs(got[k] - ref[k]).max(initial=0.0)) for k in C.KEYS}


# ------------------------------------------------------------------------------------------------
# 1. fp32 over the grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inv_s,cos_anneal', C.GRID)
def test_fp32_forward_and_backward_are_within_the_yardstick(inv_s, cos_anneal):
    res, ref = _run(inv_s, cos_anneal, torch.float32), C.reference(inv_s, cos_anneal)
    errs = _errors(res, ref)
    print(f'PARITY sdf_sigmas inv_s {inv_s:g} cos_anneal {cos_anneal:.1f}: ' +
          ', '.join(f'{k} {errs[k]:.3g} (bound {C.yardstick(k)[0]:.3g}, float32 CPU {C.yardstick(k)[1]:.3g})' for k in C.KEYS))
    for k in C.KEYS:
        assert errs[k] <= C.yardstick(k)[0], (k, errs[k], C.yardstick(k))
    assert all(torch.isfinite(res[k]).all() for k in res)
    # capped rows: the cap itself, and exactly no gradient; padding rows: exactly no density and no gradient
    t = C.sample_table()
    cap, pad = torch.from_numpy(ref['capped']).cuda(), torch.from_numpy(t['deltas'][:, 0] == 0).cuda()
    assert _bits_equal(res['sigma'][cap], (torch.tensor(C.X_MAX, dtype=torch.float32, device='cuda') / cu(t['deltas'][:, 0], torch.float32))[cap])
    assert (res['sigma'][pad] == 0).all() and int(pad.sum()) == C.M - C.LIVE
    for k in ('grad_sdf', 'grad_normals', 'grad_dirs'):
        assert (res[k][cap] == 0).all() and (res[k][pad] == 0).all(), k
        assert (res[k][~(cap | pad)] != 0).any(), k


def test_backward_is_bit_reproducible():
    for inv_s, cos_anneal in ((64.0, C.COS_ANNEAL[1]), (3000.0, 1.0)):
        a, b = _run(inv_s, cos_anneal, torch.float32), _run(inv_s, cos_anneal, torch.float32)
        for k in a:
            assert _bits_equal(a[k], b[k]), (inv_s, k)


# ------------------------------------------------------------------------------------------------
# 2. row counts: below / at / above a wave and a workgroup; every one a prefix of the full run
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [0, 1, 63, 64, 65, 257, 1600])
def test_row_count_prefix_is_bit_identical_to_the_full_run(rows):
    inv_s, cos_anneal = 512.0, C.COS_ANNEAL[1]
    full, part = _run(inv_s, cos_anneal, torch.float32), _run(inv_s, cos_anneal, torch.float32, rows=rows)
    for k in ('sigma', 'grad_sdf', 'grad_normals', 'grad_dirs'):
        assert part[k].shape[0] == rows and _bits_equal(part[k], full[k][:rows]), k
    if rows == 0:
        assert part['grad_inv_s'].shape == (1,) and float(part['grad_inv_s']) == 0.0
    else:   # a sum over the rows: against float64 on the same prefix
        ref = C.evaluate(inv_s, cos_anneal, torch.float64, rows=rows)
        err = abs(float(part['grad_inv_s']) - float(ref['grad_inv_s'][0]))
        assert err <= C.yardstick('grad_inv_s')[0], (rows, err)


# ------------------------------------------------------------------------------------------------
# 3. dtypes
# ------------------------------------------------------------------------------------------------
def _close(got, want, rel=1e-12):
    """the tolerance of tests/test_gpu_fp64.py::_close"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want)
    bound = rel * np.abs(want) + rel * 1e-2 * max(1.0, float(np.abs(want).max(initial=0.0)))
    bad = err > bound
    assert not bad.any(), (int(bad.sum()), float(err.max()), got[bad][:4], want[bad][:4])


def test_fp64_matches_the_definition():
    for inv_s, cos_anneal in C.GRID:
        res, ref = _run(inv_s, cos_anneal, torch.float64), C.reference(inv_s, cos_anneal)
        assert all(v.dtype == torch.float64 for v in res.values())
        for k in ('sigma',) + GRAD_KEYS:
            _close(res[k].cpu().numpy(), ref[k])


def test_fp64_gradcheck_including_inv_s():
    import raymarching
    inv_s, cos_anneal = 64.0, C.COS_ANNEAL[1]
    t = C.sample_table()
    assert not C.reference(inv_s, cos_anneal)['capped'][:64].any()
    leaf = lambda k: cu(t[k][:64], torch.float64).requires_grad_(True)
    deltas = cu(t['deltas'][:64], torch.float64)
    s = torch.tensor([inv_s], dtype=torch.float64, device='cuda', requires_grad=True)
    fn = lambda sdf, normals, dirs, s: raymarching.sdf_sigmas(sdf, normals, dirs, deltas, s, cos_anneal)
    assert torch.autograd.gradcheck(fn, (leaf('sdf'), leaf('normals'), leaf('dirs'), s), eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)


def test_fp16_inputs_under_autocast_give_the_fp32_result_of_the_upcast_inputs():
    inv_s, cos_anneal = 64.0, 1.0
    with torch.autocast('cuda', dtype=torch.float16):
        half = _run(inv_s, cos_anneal, torch.float32, cast=torch.float16)
    import raymarching
    t = C.sample_table()
    up16 = lambda k, grad=True: cu(t[k], torch.float32).half().float().requires_grad_(grad)
    sdf, normals, dirs, deltas = up16('sdf'), up16('normals'), up16('dirs'), up16('deltas', False)
    s = torch.tensor([inv_s], dtype=torch.float32, device='cuda', requires_grad=True)
    sigma = raymarching.sdf_sigmas(sdf, normals, dirs, deltas, s, cos_anneal)
    sigma.backward(cu(t['up'], torch.float32))
    assert half['sigma'].dtype == torch.float32 and _bits_equal(half['sigma'], sigma.detach())
    assert _bits_equal(half['grad_inv_s'], s.grad)
    for k, g in (('grad_sdf', sdf.grad), ('grad_normals', normals.grad), ('grad_dirs', dirs.grad)):
        assert half[k].dtype == torch.float16 and _bits_equal(half[k], g.half()), k   # the fp32 gradient, rounded once on the way to the fp16 leaf


# ------------------------------------------------------------------------------------------------
# 4. behaviour
# ------------------------------------------------------------------------------------------------
def test_dirs_gradient_only_when_dirs_require_it():
    inv_s, cos_anneal = 64.0, C.COS_ANNEAL[1]
    with_dirs, without = _run(inv_s, cos_anneal, torch.float32), _run(inv_s, cos_anneal, torch.float32, dirs_grad=False)
    assert without['grad_dirs'] is None and with_dirs['grad_dirs'] is not None
    for k in ('sigma', 'grad_sdf', 'grad_normals', 'grad_inv_s'):
        assert _bits_equal(with_dirs[k], without[k]), k


def test_second_order_raises():
    import raymarching
    t = C.sample_table()
    sdf = cu(t['sdf'][:64], torch.float32).requires_grad_(True)
    s = torch.tensor([64.0], device='cuda', requires_grad=True)
    sigma = raymarching.sdf_sigmas(sdf, cu(t['normals'][:64], torch.float32), cu(t['dirs'][:64], torch.float32), cu(t['deltas'][:64], torch.float32), s, 1.0)
    with pytest.raises(RuntimeError, match='second-order'):
        torch.autograd.grad((sigma ** 2).sum(), sdf, create_graph=True)


# ------------------------------------------------------------------------------------------------
# 5. composed with the compositors the project already has
# ------------------------------------------------------------------------------------------------
def test_composited_sdf_rays_match_the_literal_neus_rendering():
    import raymarching
    r, lit = C.ray_case(), C.ray_literal()
    f32 = lambda k: cu(r[k], torch.float32)
    s = torch.tensor([C.RAY_INV_S], device='cuda')
    sigmas = raymarching.sdf_sigmas(f32('sdf'), f32('normals'), f32('dirs'), f32('deltas'), s, C.RAY_COS_ANNEAL)
    weights_sum, _, image = raymarching.composite_rays_train(sigmas, f32('rgbs'), f32('deltas'), cu(r['rays']), G.T_THRESH)
    geo = raymarching.composite_rays_train_geo(sigmas, f32('rgbs'), f32('deltas'), cu(r['rays']), G.T_THRESH)
    got = dict(weights_sum=weights_sum, image=image, depth=geo[1])
    for k in ('weights_sum', 'image', 'depth'):
        err = float(np.abs(got[k].double().cpu().numpy() - lit[k]).max())
        bound, f32_err = C.ray_yardstick(k)
        print(f'PARITY sdf_sigmas -> compositor: {k} {err:.3g} (bound {bound:.3g}, float32 CPU {f32_err:.3g})')
        assert err <= bound, (k, err, bound)
    assert _bits_equal(geo[0], weights_sum) and _bits_equal(geo[2], image)
