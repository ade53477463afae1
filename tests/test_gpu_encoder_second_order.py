"""GPU: second order through the frequency and the SH encoder (csrc/encoder_second.hip) and the fp64 frequency encoder.

Reference: float64 pure-PyTorch statements (tests/encoder_second_cases.py) differentiated by autograd on the fp32-rounded inputs -- the
frequency encoder twice through autograd.grad, the SH basis as its autograd Jacobian and Hessian (of sympy.lambdify(gen_sh.basis()), the
differentiation is autograd's), computed once for the largest batch and sliced.

Tolerances.  fp64: 1e-10 of the sum of the absolute terms of a point's row (fp64 kernels on rows of at most 63 terms with factors up to
4^9; sin(2^f x + pi/2) for cos carries an absolute error of ~2^f * 1.1e-16, which is why the scale is the row and not the element).
fp32, "as implemented" (the reference is fed the kernel's own stored outputs / dy_dx): one rounding of 2^-24 per operation, bounds stated
at each test.  fp32 SH dL/dx against the float64 reference: measured on the MI355X, see test_sh_fp32_grad_inputs2_against_float64."""
import functools

import pytest
import torch

from encoder_second_cases import (BATCHES, EPS32, FREQ_SHAPES, SH_DEGREES, freq_reference, sh_functions, sh_reference, three_orders,
                                  unit_vectors)

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BMAX = max(BATCHES)
WIDE = (700, 3)   # C = 4900: wider than the LDS tile of k_freq_bwd_bwd in fp32 and fp64 -> k_freq_bwd_bwd_wide


def _rand(shape, seed, lo=-1.0, hi=1.0):
    """fp32-representable values, as float64"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=F64) * (hi - lo) + lo).to(F32).to(F64)


# ---- references (CPU, float64), once per shape ---------------------------------------------------------------------------------------
def _freq_slots(D, deg):
    sin = torch.tensor([D + 2 * f * D + d for f in range(deg) for d in range(D)], dtype=torch.long).view(deg, D)
    return sin, sin + D


def _freq_formulas(o, w, v, D, deg):
    """the second order as the kernel forms it from stored outputs o (float64 arithmetic): dL/dw, dL/dx, and for each the sum of the
    absolute terms (element-wise for dL/dw: a single term; per (b, d) for dL/dx: |v_d| sum_f 4^f (|w_sin o_sin| + |w_cos o_cos|))"""
    B = o.shape[0]
    dw = torch.zeros_like(o)
    dw[:, :D] = v
    dx = torch.zeros(B, D, dtype=F64)
    dx_abs = torch.zeros(B, D, dtype=F64)
    if deg:
        s, c = _freq_slots(D, deg)
        scale = (2.0 ** torch.arange(deg, dtype=F64)).view(1, deg, 1)
        dw[:, s.flatten()] = (scale * v[:, None, :] * o[:, c.flatten()].view(B, deg, D)).view(B, -1)
        dw[:, c.flatten()] = (-scale * v[:, None, :] * o[:, s.flatten()].view(B, deg, D)).view(B, -1)
        ws, wc, os_, oc = (t[:, i.flatten()].view(B, deg, D) for t, i in ((w, s), (w, c), (o, s), (o, c)))
        dx = -v * (scale ** 2 * (ws * os_ + wc * oc)).sum(1)
        dx_abs = v.abs() * (scale ** 2 * ((ws * os_).abs() + (wc * oc).abs())).sum(1)
    return dw, dx, dx_abs


@functools.lru_cache(maxsize=None)
def _freq_case(D, deg, B=BMAX):
    C = D * (1 + 2 * deg)
    x, w, v = _rand((B, D), 1), _rand((B, C), 2), _rand((B, D), 3)
    y, gx, dw, dx = three_orders(lambda t: freq_reference(t, deg), x.clone().requires_grad_(True), w.clone().requires_grad_(True), v)
    # sums of absolute terms per row
    gx_abs = w[:, :D].abs().clone()
    if deg:
        s, c = _freq_slots(D, deg)
        scale = (2.0 ** torch.arange(deg, dtype=F64)).view(1, deg, 1)
        t = lambda a, i: a[:, i.flatten()].view(B, deg, D)
        gx_abs = gx_abs + (scale * ((t(w, s) * t(y, c)).abs() + (t(w, c) * t(y, s)).abs())).sum(1)
    _, _, dx_abs = _freq_formulas(y, w, v, D, deg)
    scales = dict(y=y.abs().sum(1), gx=gx_abs.sum(1), dw=dw.abs().sum(1), dx=dx_abs.sum(1))
    return dict(x=x, w=w, v=v, y=y, gx=gx, dw=dw, dx=dx, scales=scales, C=C)


@functools.lru_cache(maxsize=None)
def _sh_basis_derivatives():
    """Y [B,64], J [B,64,3] and H [B,64,3,3] of the basis at BMAX unit vectors (fp32-rounded): autograd, twice, one polynomial at a time
    on separate coordinate leaves (small graphs)"""
    p = unit_vectors(BMAX, seed=5, dtype=F32).to(F64)
    xyz = [c.clone().requires_grad_(True) for c in p.unbind(-1)]
    Y = sh_reference(p, 8)
    J = torch.zeros(BMAX, 64, 3, dtype=F64)
    H = torch.zeros(BMAX, 64, 3, 3, dtype=F64)
    for i, f in enumerate(sh_functions()):
        yi = f(*xyz)
        if not torch.is_tensor(yi):   # the constant
            continue
        g = torch.autograd.grad(yi.sum(), xyz, create_graph=True, allow_unused=True)
        for d in range(3):
            if g[d] is None:
                continue
            J[:, i, d] = g[d].detach()
            if g[d].requires_grad:
                for e, h in enumerate(torch.autograd.grad(g[d].sum(), xyz, retain_graph=True, allow_unused=True)):
                    if h is not None:
                        H[:, i, d, e] = h
    return p, Y, J, H


@functools.lru_cache(maxsize=None)
def _sh_case(degree):
    N = degree * degree
    p, Y, J, H = _sh_basis_derivatives()
    Y, J, H = Y[:, :N], J[:, :N], H[:, :N]
    w, v = _rand((BMAX, N), 20 + degree), _rand((BMAX, 3), 40 + degree)
    gx = torch.einsum('bi,bid->bd', w, J)
    dw = torch.einsum('bd,bid->bi', v, J)
    dx = torch.einsum('bi,bd,bide->be', w, v, H)
    scales = dict(y=Y.abs().sum(1), gx=torch.einsum('bi,bid->b', w.abs(), J.abs()), dw=torch.einsum('bd,bid->b', v.abs(), J.abs()),
                  dx=torch.einsum('bi,bd,bide->b', w.abs(), v.abs(), H.abs()))
    return dict(x=p, w=w, v=v, y=Y, gx=gx, dw=dw, dx=dx, scales=scales, J=J)


def _assert_rows(got, want, scale, rtol, what):
    err = (got.detach().cpu().to(F64) - want).abs().amax(1)
    bound = rtol * scale
    assert bool((err <= bound).all()), f'{what}: error {float(err.max()):.3g}, worst error / row scale {float((err / scale.clamp_min(1e-300)).max()):.3g} > {rtol}'


def _module_three_orders(fn, case, B, dtype):
    x = case['x'][:B].to(dtype).cuda().requires_grad_(True)
    w = case['w'][:B].to(dtype).cuda().requires_grad_(True)
    return three_orders(fn, x, w, case['v'][:B].to(dtype).cuda())


# ---- 1. fp64 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,deg', [(3, 4), (2, 6)])
def test_fp64_freq_gradcheck_and_gradgradcheck(D, deg):
    from freqencoder import freq_encode
    x = _rand((5, D), 7).cuda().requires_grad_(True)
    fn = lambda t: freq_encode(t, deg, D * (1 + 2 * deg))
    assert fn(x).dtype == F64
    assert torch.autograd.gradcheck(fn, (x,), nondet_tol=0.0)
    assert torch.autograd.gradgradcheck(fn, (x,), nondet_tol=0.0)


@pytest.mark.parametrize('degree', [2, 4, 8])
def test_fp64_sh_gradcheck_and_gradgradcheck(degree):
    from shencoder import sh_encode
    x = unit_vectors(5, seed=8).cuda().requires_grad_(True)
    fn = lambda t: sh_encode(t, degree, True)
    assert torch.autograd.gradcheck(fn, (x,), nondet_tol=0.0)
    assert torch.autograd.gradgradcheck(fn, (x,), nondet_tol=0.0)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('D,deg', FREQ_SHAPES)
def test_fp64_freq_three_orders_match_float64_autograd(D, deg, B):
    from freqencoder import freq_encode
    case = _freq_case(D, deg)
    got = _module_three_orders(lambda t: freq_encode(t, deg, case['C']), case, B, F64)
    for name, g in zip(('y', 'gx', 'dw', 'dx'), got):
        assert g.dtype == F64
        _assert_rows(g, case[name][:B], case['scales'][name][:B], 1e-10, f'freq D={D} deg={deg} B={B} {name}')


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('degree', SH_DEGREES)
def test_fp64_sh_three_orders_match_float64_autograd(degree, B):
    from shencoder import sh_encode
    case = _sh_case(degree)
    got = _module_three_orders(lambda t: sh_encode(t, degree, True), case, B, F64)
    for name, g in zip(('y', 'gx', 'dw', 'dx'), got):
        assert g.dtype == F64
        _assert_rows(g, case[name][:B], case['scales'][name][:B], 1e-10, f'sh degree={degree} B={B} {name}')
    if degree == 1:   # constant outputs: both second-order results are zeros
        assert not got[2].any() and not got[3].any()


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_freq_rows_wider_than_the_tile(dtype):
    """C = 4900 elements do not fit k_freq_bwd_bwd's LDS tile: the straight-from-memory kernel, same arithmetic.  fp64: as above; fp32: 1e-3
    of each tensor's maximum would be the parity bar -- here the fp32 result is held to the as-implemented bounds of the tiled kernel"""
    import freqencoder.freq as fq
    D, deg = WIDE
    case = _freq_case(D, deg, 3)
    C = case['C']
    if dtype == F64:
        got = _module_three_orders(lambda t: fq.freq_encode(t, deg, C), case, 3, F64)
        for name, g in zip(('y', 'gx', 'dw', 'dx'), got):
            _assert_rows(g, case[name], case['scales'][name], 1e-10, f'wide freq {name}')
    else:
        _check_freq_fp32_as_implemented(D, deg, 3, case)


# ---- 2. fp32, as implemented ----------------------------------------------------------------------------------------------------------------
def _check_freq_fp32_as_implemented(D, deg, B, case):
    import freqencoder.freq as fq
    C = case['C']
    x, w, v = (case[k][:B].to(F32).cuda() for k in ('x', 'w', 'v'))
    o = torch.empty(B, C, device='cuda')
    fq._backend.freq_encode_forward(x, B, D, deg, C, o)
    dw, dx = torch.full((B, C), float('nan'), device='cuda'), torch.full((B, D), float('nan'), device='cuda')
    fq.freq_encode_backward_backward(w, o, v, B, D, deg, C, dw, dx)
    want_dw, want_dx, dx_abs = _freq_formulas(o.cpu().to(F64), case['w'][:B], case['v'][:B], D, deg)
    # dL/dg: a single rounded product after an exact power-of-two scale
    assert bool(((dw.cpu().to(F64) - want_dw).abs() <= EPS32 * want_dw.abs()).all())
    # dL/dx: products, the pair sum, deg fused multiply-adds, the final product: (2 deg + 3) 2^-23 of the sum of the absolute terms
    err = (dx.cpu().to(F64) - want_dx).abs()
    assert bool((err <= (2 * deg + 3) * EPS32 * dx_abs).all()), float((err / dx_abs.clamp_min(1e-300)).max() / EPS32)
    # the optional outputs: each alone gives the same bits
    dw1, dx1 = torch.empty_like(dw), torch.empty_like(dx)
    fq.freq_encode_backward_backward(w, o, v, B, D, deg, C, dw1, None)
    fq.freq_encode_backward_backward(w, o, v, B, D, deg, C, None, dx1)
    assert torch.equal(dw1, dw) and torch.equal(dx1, dx)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('D,deg', FREQ_SHAPES)
def test_fp32_freq_as_implemented(D, deg, B):
    _check_freq_fp32_as_implemented(D, deg, B, _freq_case(D, deg))


def _sh_fp32_call(degree, B):
    import shencoder.sphere_harmonics as sh
    case = _sh_case(degree)
    N = degree * degree
    x, w, v = (case[k][:B].to(F32).cuda() for k in ('x', 'w', 'v'))
    y, dy_dx = torch.empty(B, N, device='cuda'), torch.empty(B, 3 * N, device='cuda')
    sh._backend.sh_encode_forward(x, y, B, 3, degree, dy_dx)
    dw, dx = torch.full((B, N), float('nan'), device='cuda'), torch.full((B, 3), float('nan'), device='cuda')
    sh.sh_encode_backward_backward(w, x, dy_dx, v, B, 3, degree, dw, dx)
    return case, (x, w, v, dy_dx), dw, dx


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('degree', SH_DEGREES)
def test_fp32_sh_grad_grad_as_implemented(degree, B):
    """dL/dg_i = sum_d u_d dy_dx[d,i] from the stored dy_dx: a product and two fused multiply-adds, 4 * 2^-23 of the sum of absolute terms"""
    import shencoder.sphere_harmonics as sh
    case, (x, w, v, dy_dx), dw, dx = _sh_fp32_call(degree, B)
    J = dy_dx.cpu().to(F64).view(B, 3, -1)
    vv = case['v'][:B]
    want, scale = torch.einsum('bd,bdi->bi', vv, J), torch.einsum('bd,bdi->bi', vv.abs(), J.abs())
    assert bool(((dw.cpu().to(F64) - want).abs() <= 4 * EPS32 * scale).all())
    dw1, dx1 = torch.empty_like(dw), torch.empty_like(dx)
    sh.sh_encode_backward_backward(w, x, dy_dx, v, B, 3, degree, dw1, None)
    sh.sh_encode_backward_backward(w, x, dy_dx, v, B, 3, degree, None, dx1)
    assert torch.equal(dw1, dw) and torch.equal(dx1, dx)
    if degree == 1:
        assert not dw.any() and not dx.any()


# ---- 3. fp32 SH dL/dx: the Hessian polynomials in fp32 --------------------------------------------------------------------------------
SH_DX_MEASURED = 2.807e-07   # largest error / largest reference magnitude of a case, measured on the MI355X (degree 5; 2.4 fp32 ulp)
SH_DX_BOUND = 4 * SH_DX_MEASURED


def test_sh_fp32_grad_inputs2_against_float64():
    """fp32 Hessian polynomials against the float64 autograd reference, unit vectors, degrees 1..8, B = 1000: the largest error of a case
    divided by the case's largest reference magnitude.  Measured on the MI355X, per degree 1..8: 0, 0, 7.2e-08, 1.3e-07, 2.8e-07, 1.9e-07,
    1.9e-07, 2.1e-07 (0.6 .. 2.4 ulp of the largest magnitude: far below the 1000 ulp at which the expression form would be at fault).  The
    largest, 2.807e-07, is SH_DX_MEASURED; the bound is four times that, 1.123e-06 (the factor covers other seeds)."""
    worst = 0.0
    for degree in SH_DEGREES:
        case, _, _, dx = _sh_fp32_call(degree, BMAX)
        err, ref = float((dx.cpu().to(F64) - case['dx']).abs().max()), float(case['dx'].abs().max())
        ratio = err / ref if ref else err
        print(f'sh degree {degree}: fp32 dL/dx error {err:.3g}, largest reference {ref:.3g}, ratio {ratio:.3g} = {ratio / EPS32:.1f} ulp')
        worst = max(worst, ratio)
    print(f'worst ratio {worst:.4g}')
    assert worst <= SH_DX_BOUND


# ---- 4. first order unchanged, determinism ------------------------------------------------------------------------------------------------
def test_first_order_bits_are_unchanged():
    from freqencoder import FreqEncoder
    from shencoder import SHEncoder
    import freqencoder.freq as fq
    import shencoder.sphere_harmonics as sh
    B = 257
    x = _rand((B, 3), 9).to(F32).cuda()
    enc = FreqEncoder(3, 6)
    w = _rand((B, enc.output_dim), 10).to(F32).cuda()
    xr = x.clone().requires_grad_(True)
    y = enc(xr)
    y.backward(w)
    o, gi = torch.empty_like(y), torch.empty(B, 3, device='cuda')
    fq._backend.freq_encode_forward(x, B, 3, 6, enc.output_dim, o)
    fq._backend.freq_encode_backward(w, o, B, 3, 6, enc.output_dim, gi)
    assert torch.equal(y.detach(), o) and torch.equal(xr.grad, gi)

    p = unit_vectors(B, seed=12, dtype=F32).cuda()
    senc = SHEncoder(degree=4)
    ws = _rand((B, 16), 13).to(F32).cuda()
    pr = p.clone().requires_grad_(True)
    ys = senc(pr)
    ys.backward(ws)
    out, dy_dx, gs = torch.empty(B, 16, device='cuda'), torch.empty(B, 48, device='cuda'), torch.zeros(B, 3, device='cuda')
    sh._backend.sh_encode_forward(p, out, B, 3, 4, dy_dx)
    sh._backend.sh_encode_backward(ws, p, B, 3, 4, dy_dx, gs)
    assert torch.equal(ys.detach(), out) and torch.equal(pr.grad, gs)
    # the differentiable first backward issues the same call: the same bits under create_graph
    (g2,) = torch.autograd.grad(senc(pr), pr, ws, create_graph=True)
    (g3,) = torch.autograd.grad(enc(xr), xr, w, create_graph=True)
    assert torch.equal(g2.detach(), gs) and torch.equal(g3.detach(), gi)
    # sh_encode(..., calc_grad_inputs=False) still returns no gradient
    from shencoder import sh_encode
    q = p.clone().requires_grad_(True)
    assert torch.autograd.grad(sh_encode(q, 4, False).sum(), q, allow_unused=True)[0] is None


# ---- 5. the silent drop is gone ---------------------------------------------------------------------------------------------------------
def test_first_backward_is_part_of_the_graph():
    from freqencoder import FreqEncoder
    from shencoder import SHEncoder
    for enc, x in ((FreqEncoder(3, 4), _rand((8, 3), 14).to(F32)), (SHEncoder(degree=4), unit_vectors(8, 15, F32))):
        x = x.cuda().requires_grad_(True)
        (gx,) = torch.autograd.grad(enc(x).sum(), x, create_graph=True)
        assert gx.requires_grad, type(enc).__name__


def _sdf_net(width_in, dtype, device):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(width_in, 64), torch.nn.Softplus(), torch.nn.Linear(64, 64), torch.nn.Softplus(),
                              torch.nn.Linear(64, 1))
    return net.to(dtype=dtype, device=device)


def _eikonal_step(encode, net, x, gt):
    x = x.clone().requires_grad_(True)
    sdf = net(encode(x))
    (g,) = torch.autograd.grad(sdf.sum(), x, create_graph=True)
    loss = (sdf - gt).abs().mean() + 0.1 * ((g.norm(dim=-1) - 1.0) ** 2).mean()
    loss.backward()
    return [p.grad for p in net.parameters()] + [x.grad]


@pytest.mark.parametrize('kind', ['frequency', 'sphere_harmonics'])
def test_eikonal_step_matches_float64_torch(kind):
    """|sdf - gt| + 0.1 (|grad_x sdf| - 1)^2 through the encoder and Linear / Softplus layers, fp32 on the backend against float64 on the
    pure-torch encoder: every parameter gradient and x.grad within 1e-3 of the tensor's maximum (the project's parity bar)"""
    from freqencoder import FreqEncoder
    from shencoder import SHEncoder
    B = 257
    if kind == 'frequency':
        enc, x, ref = FreqEncoder(3, 6), _rand((B, 3), 16), (lambda t: freq_reference(t, 6))
    else:
        enc, x, ref = SHEncoder(degree=4), unit_vectors(B, 17, F32).to(F64), (lambda t: sh_reference(t, 4))
    gt = _rand((B, 1), 18)
    net64 = _sdf_net(enc.output_dim, F64, 'cpu')
    net32 = _sdf_net(enc.output_dim, F32, 'cuda')
    net32.load_state_dict({k: v.to(F32) for k, v in net64.state_dict().items()})
    want = _eikonal_step(ref, net64, x, gt)
    got = _eikonal_step(enc, net32, x.to(F32).cuda(), gt.to(F32).cuda())
    for g, r in zip(got, want):
        assert g is not None and r is not None
        assert float((g.cpu().to(F64) - r).abs().max()) <= 1e-3 * float(r.abs().max()), (kind, tuple(r.shape))


# ---- 6. autocast, unused results, third order, fp16 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['frequency', 'sphere_harmonics'])
def test_autocast_delivers_the_second_order_gradient_to_the_callers_tensor(kind):
    """the caller's fp16 tensor receives dL/dx in fp16.  Against float64 at the fp16 points: gx and x.grad are each rounded to fp16 once
    (2^-11), the loss (gx^2) doubles the first: 2^-8 of the tensor's maximum is generous"""
    from freqencoder import FreqEncoder
    from shencoder import SHEncoder
    if kind == 'frequency':
        enc, x, ref = FreqEncoder(3, 4), _rand((65, 3), 19), (lambda t: freq_reference(t, 4))
    else:
        enc, x, ref = SHEncoder(degree=4), unit_vectors(65, 20), (lambda t: sh_reference(t, 4))
    x16 = x.to(torch.float16).cuda().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = enc(x16)
        (gx,) = torch.autograd.grad(y.sum(), x16, create_graph=True)
    assert gx.requires_grad and gx.dtype == torch.float16
    (gx.float() ** 2).sum().backward()
    assert x16.grad is not None and x16.grad.dtype == torch.float16
    x64 = x16.detach().cpu().to(F64).requires_grad_(True)
    (g64,) = torch.autograd.grad(ref(x64).sum(), x64, create_graph=True)
    (want,) = torch.autograd.grad((g64 ** 2).sum(), x64)
    assert float(want.abs().max()) > 1.0
    assert float((x16.grad.cpu().to(F64) - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())


@pytest.mark.parametrize('kind', ['frequency', 'sphere_harmonics'])
def test_unused_results_launch_nothing_and_third_order_raises(kind, monkeypatch):
    import freqencoder.freq as fq
    import shencoder.sphere_harmonics as sh
    if kind == 'frequency':
        mod, name, enc, x = fq, 'freq_encode_backward_backward', fq.FreqEncoder(3, 4), _rand((65, 3), 21).to(F32)
    else:
        mod, name, enc, x = sh, 'sh_encode_backward_backward', sh.SHEncoder(degree=4), unit_vectors(65, 22, F32)
    calls, inner = [], getattr(mod, name)

    def counted(*args):
        calls.append(args)
        return inner(*args)
    monkeypatch.setattr(mod, name, counted)
    x = x.cuda().requires_grad_(True)
    y = enc(x)
    (gx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    (y * y).sum().backward(retain_graph=True)      # a loss that does not use gx: u is None, nothing is launched
    assert calls == [] and x.grad is not None
    (h,) = torch.autograd.grad((gx ** 2).sum(), x, create_graph=True)
    assert len(calls) == 1
    grad_grad, grad_inputs2 = calls[0][-2:]
    assert grad_grad is None and grad_inputs2 is not None   # the upstream gradient (ones) needs no gradient: NULL for that output
    assert h.requires_grad
    with pytest.raises(RuntimeError, match='third-order gradients are not provided'):
        torch.autograd.grad(h.sum(), x)


def test_fp16_tensors_are_refused_by_the_sh_entry():
    import _ngp_capi as capi
    t = lambda *s: torch.zeros(*s, dtype=torch.float16, device='cuda')
    g, x, dy_dx, u, gg, gi = t(8, 16), t(8, 3), t(8, 48), t(8, 3), t(8, 16), t(8, 3)
    rc = capi.lib.ngp_sh_encode_backward_backward(g.data_ptr(), x.data_ptr(), dy_dx.data_ptr(), u.data_ptr(), 8, 3, 4, gg.data_ptr(), gi.data_ptr(),
                                                  capi.float_code(g, 'grad'), capi.stream())
    assert rc == 1 and b'second order is provided for float32 and float64' in capi.lib.ngp_last_error()
    import shencoder.sphere_harmonics as sh
    with pytest.raises(RuntimeError, match='second order is provided for float32 and float64'):
        sh.sh_encode_backward_backward(g, x, dy_dx, u, 8, 3, 4, gg, gi)


def test_new_entries_are_deterministic():
    """two calls of each new entry on the same inputs are bit-identical (no atomics, fixed summation order)"""
    import _ngp_capi as capi
    import freqencoder.freq as fq
    import shencoder.sphere_harmonics as sh
    B = 1000
    for dtype in (F32, F64):
        case = _freq_case(3, 10)
        x, w, v = (case[k].to(dtype).cuda() for k in ('x', 'w', 'v'))
        runs = []
        for _ in range(2):
            o = torch.empty(B, 63, dtype=dtype, device='cuda')
            fq._forward_call(x, B, 3, 10, 63, o)
            gi = fq._first_order_backward(w, o, (B, 3, 10, 63))
            dw, dx = torch.empty_like(o), torch.empty_like(x)
            fq.freq_encode_backward_backward(w, o, v, B, 3, 10, 63, dw, dx)
            runs.append((o, gi, dw, dx))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), dtype
        case = _sh_case(8)
        x, w, v = (case[k].to(dtype).cuda() for k in ('x', 'w', 'v'))
        y, dy_dx = torch.empty(B, 64, dtype=dtype, device='cuda'), torch.empty(B, 192, dtype=dtype, device='cuda')
        sh._backend.sh_encode_forward(x, y, B, 3, 8, dy_dx)
        runs = []
        for _ in range(2):
            dw, dx = torch.empty_like(y), torch.empty_like(x)
            sh.sh_encode_backward_backward(w, x, dy_dx, v, B, 3, 8, dw, dx)
            runs.append((dw, dx))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), dtype
    assert capi.lib.ngp_abi_version() == 11
