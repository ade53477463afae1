"""Second order through the FFMLP (ffmlp/ffmlp.py _ffmlp_backward, csrc/ffmlp_second.inc): ngp_ffmlp_backward_backward against the
float64 reference of tests/ffmlp_second_cases.py at the kernels' rounding points, over the whole case table; exact zeros where f' = 0;
bit reproducibility; NULL outputs; the module under autocast (unchanged first order, an eikonal loss, an eikonal plus a data term); a
hash grid feeding the MLP against a float64 pure-PyTorch statement differentiated twice; the refusals.

Bars (tests/ffmlp_act_cases.py, the first order's): dL/dg and dL/dx |got - ref| <= 4e-3 (|ref| + max |ref|) on every element; dL/dW per
matrix relative L2 < 2e-3 and max error < 3e-3 of the maximum.  The reference rounds where the kernels round (d, p, q, s), so what is
left is fp32 against float64 accumulation, __expf, and roundings that flip -- the same kind of residual as in the first order."""
import ctypes

import numpy as np
import pytest
import torch

import oracle

import ffmlp_act_cases as A
import ffmlp_second_cases as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _capi():
    import _ngp_capi as capi
    return capi


def cu16(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(DEV).half().contiguous()


def _forward(xt, wt, B, din, hid, nl, act):
    capi = _capi()
    out = torch.empty(B, 16, device=DEV, dtype=torch.half)
    fb = torch.empty(nl, B, hid, device=DEV, dtype=torch.half)
    capi.check(capi.lib.ngp_ffmlp_forward(xt.data_ptr(), wt.data_ptr(), B, din, 16, hid, nl, act, 6, fb.data_ptr(), out.data_ptr(), capi.stream()))
    return fb


def _second(gt, xt, wt, fb, ut, B, din, hid, nl, act, want=(True, True, True)):
    """-> (grad_grad, grad_weights2, grad_inputs2) fp16 tensors, None where not asked for; they start as NaN so that anything left
    unwritten shows"""
    capi = _capi()
    nan = lambda *shape: torch.full(shape, float('nan'), device=DEV, dtype=torch.half)
    outs = [nan(B, 16) if want[0] else None, nan(A.n_params(din, hid, nl)) if want[1] else None, nan(B, din) if want[2] else None]
    nbytes = int(capi.lib.ngp_ffmlp_backward_backward_workspace_bytes(B, din, hid, nl, act))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    capi.check(capi.lib.ngp_ffmlp_backward_backward(gt.data_ptr(), xt.data_ptr(), wt.data_ptr(), fb.data_ptr(), ut.data_ptr(), B, din, 16, hid, nl,
                                                    act, capi.ptr(outs[0]), capi.ptr(outs[1]), capi.ptr(outs[2]), ws.data_ptr(), nbytes,
                                                    capi.stream()))
    torch.cuda.synchronize()
    return outs


def _run_case(din, hid, nl, act, B, want=(True, True, True)):
    c = S.case(din, hid, nl, act, B)
    S.check_conditions(c, din, hid, nl, act)
    xt, wt, gt, ut = cu16(c['x']), cu16(c['w']), cu16(c['g']), cu16(c['u'])
    fb = _forward(xt, wt, B, din, hid, nl, act)
    return c, (gt, xt, wt, fb, ut), _second(gt, xt, wt, fb, ut, B, din, hid, nl, act, want)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _check(label, dg, gw, dx, ref_dg, ref_gw, ref_dx, din, hid, nl, act, bars):
    """every figure is printed before anything is asserted"""
    bar_dg, bar_dx, bar_l2, bar_max = bars
    e_dg = A.dx_errors(dg, ref_dg) if dg is not None else (0.0, 0.0)   # (dg None: not part of this comparison)
    werr = A.w_errors(gw, ref_gw, din, hid, nl)
    sloped = act in S.SLOPED
    e_dx = A.dx_errors(dx, ref_dx) if sloped else (float(np.abs(dx).max()), 0.0)
    print(f'PARITY second {label}: dg elem {e_dg[0]:.2e} max {e_dg[1]:.2e} | dx elem {e_dx[0]:.2e} max {e_dx[1]:.2e} | '
          f'dW L2 {max(w[0] for w in werr):.2e} max {max(w[1] for w in werr):.2e}')
    assert np.isfinite(gw).all() and np.isfinite(dx).all(), label
    if dg is not None:
        assert np.isfinite(dg).all(), label
        assert (np.abs(dg - ref_dg) <= bar_dg * (np.abs(ref_dg) + np.abs(ref_dg).max())).all(), (label, 'dg', e_dg)
    if sloped:
        assert (np.abs(dx - ref_dx) <= bar_dx * (np.abs(ref_dx) + np.abs(ref_dx).max())).all(), (label, 'dx', e_dx)
    else:
        assert not dx.any(), (label, 'dx must be exactly zero')
    for l2, mx in werr:
        assert l2 < bar_l2 and mx < bar_max, (label, werr)


def _id(v):
    return '-'.join(str(x) for x in v)


@pytest.mark.parametrize('case', S.CASES, ids=_id)
@pytest.mark.parametrize('B', S.BATCHES)
def test_capi_against_the_rounded_reference(case, B):
    """k_ffmlp_dgrad_layered, k_ffmlp_tangent_layered, k_ffmlp_dgrad2_layered (f' != 0), k_ffmlp_wgrad twice, k_ffmlp_reduce_slabs for
    widths 16 / 32 / 64 / 128 / 256, 16 .. 96 inputs, 2 .. 5 layers; for ReLU, Sine and None dL/dx is exactly zero"""
    din, hid, nl, act = case
    c, _, (dg, gw, dx) = _run_case(din, hid, nl, act, B)
    _check(f'{din}->{hid}x{nl} {S.ACT_NAMES[act]} B={B}', _np(dg), _np(gw), _np(dx), c['dg'], c['gw'], c['dx'], din, hid, nl, act,
           S.bars(din, hid, nl, act, B))


REPEAT_CASES = [(32, 64, 3, 5, 4224), (48, 256, 3, 6, 4224), (32, 16, 2, 5, 128), (32, 64, 3, 0, 4224)]


@pytest.mark.parametrize('case', REPEAT_CASES, ids=_id)
def test_two_calls_are_bit_identical(case):
    din, hid, nl, act, B = case
    _, args, first = _run_case(din, hid, nl, act, B)
    again = _second(*args, B, din, hid, nl, act)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize('case', REPEAT_CASES[:3], ids=_id)
def test_null_outputs_skip_their_terms_and_leave_the_others_bit_identical(case):
    din, hid, nl, act, B = case
    _, args, full = _run_case(din, hid, nl, act, B)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        part = _second(*args, B, din, hid, nl, act, want)
        for asked, a, b in zip(want, part, full):
            assert (a is None) if not asked else torch.equal(a, b), want
    # no output at all: nothing to do, nothing touched
    assert _second(*args, B, din, hid, nl, act, (False, False, False)) == [None, None, None]


# ---- module level: FFMLP(32, 1, 64, 3, 'softplus') under autocast, B = 256 (padded to 384 rows inside the module) ----

def _module():
    from ffmlp import FFMLP
    din, hid, nl, act = S.MODULE_CASE
    _, x, w = A._inputs(din, hid, nl, act, S.MODULE_B)
    net = FFMLP(din, 1, hid, nl, activation='softplus').to(DEV)
    assert net.activation == act
    with torch.no_grad():
        net.weights.copy_(torch.tensor(w))
    return net, x, w


def _eikonal(gx):
    return ((gx.norm(dim=-1) - 1) ** 2).mean()


def _module_reference(x, w):
    """the padded problem the kernels see and a power-of-two loss scale, from the oracle alone: g is column 0 of the 16 padded outputs,
    u the eikonal loss's gradient at the oracle's grad_inputs; 2^k puts the unrounded max |dL/dx| into (1/4, 1/2]"""
    din, hid, nl, act = S.MODULE_CASE
    B, pad = S.MODULE_B, S.MODULE_B + 128
    xp = np.zeros((pad, din))
    xp[:B] = x
    g = np.zeros((pad, 16))
    g[:B, 0] = 1.0
    _, rfb = oracle.ffmlp_forward(xp, w, din, 16, hid, nl, activation=act)
    gx, _ = oracle.ffmlp_backward(g, xp, w, rfb, din, 16, hid, nl, activation=act)
    n = np.linalg.norm(gx[:B], axis=-1, keepdims=True)
    u = np.zeros((pad, din))
    u[:B] = 2 * (n - 1) / B * gx[:B] / n
    r = S.reference(g, xp, w, rfb, u, din, hid, nl, act, False)
    k = S._pow2_into_half(np.abs(r['dx']).max())
    return xp, g, rfb, k


def test_module_first_order_is_bit_identical_under_create_graph():
    net, x, _ = _module()
    xt = torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = net(xt)
    gx0, gw0 = torch.autograd.grad(y.sum(), (xt, net.weights), retain_graph=True)
    gx1, gw1 = torch.autograd.grad(y.sum(), (xt, net.weights), create_graph=True)
    assert gx1.requires_grad and not gx0.requires_grad
    assert torch.equal(gx0, gx1.detach()) and torch.equal(gw0, gw1.detach())
    assert gx0.abs().max() > 0


def test_module_eikonal_loss_fills_weight_and_input_gradients():
    """the reference takes what the op took: x, w, g = column 0, and u = d loss / d grad_inputs as autograd handed it over (a hook on
    grad_inputs; the eikonal formula itself is PyTorch's).  The loss is scaled by a power of two taken from the oracle, as a GradScaler
    would, so that dL/dx is compared in fp16's normal range."""
    din, hid, nl, act = S.MODULE_CASE
    B = S.MODULE_B
    net, x, w = _module()
    xp, g, rfb, k = _module_reference(x, w)
    xt = torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = net(xt)
        gx = torch.autograd.grad(y.sum(), xt, create_graph=True)[0]
    seen = {}
    gx.register_hook(lambda t: seen.setdefault('u', t.detach().clone()))
    (_eikonal(gx) * 2.0 ** k).backward()
    u = np.zeros_like(xp)
    u[:B] = _np(seen['u'].half())
    ref = S.reference(g, xp, w, rfb, u, din, hid, nl, act, True)
    a = np.abs(ref['dx'])
    assert 2.0 ** -3 <= a.max() <= 1.0 and np.abs(ref['gw']).max() < 2.0 ** 15, (float(a.max()), float(np.abs(ref['gw']).max()))
    assert xt.grad is not None and net.weights.grad is not None
    # (g = ones does not require grad: d loss / d g is not asked for)
    _check('module eikonal', None, _np(net.weights.grad), _np(xt.grad), None, ref['gw'], ref['dx'][:B], din, hid, nl, act,
           (S.DX_TOL, S.DX_TOL, S.W_L2, S.W_MAX))


def test_module_eikonal_plus_data_term_is_the_sum_of_both():
    """both terms reach the weights and the inputs: each gradient is one fp16 result per term, cast to fp32 and added once, whichever way
    the terms are combined"""
    net, x, w = _module()
    _, _, _, k = _module_reference(x, w)
    target = torch.linspace(-1, 1, S.MODULE_B, device=DEV)[:, None]

    def grads(eik, data):
        net.zero_grad()
        xt = torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True)
        with torch.autocast('cuda', dtype=torch.float16):
            y = net(xt)
            gx = torch.autograd.grad(y.sum(), xt, create_graph=True)[0]
        loss = 0.0
        if eik:
            loss = loss + _eikonal(gx) * 2.0 ** k
        if data:
            loss = loss + ((y.float() - target) ** 2).mean() * 64.0
        loss.backward()
        return xt.grad.clone(), net.weights.grad.clone()

    ex, ew = grads(True, False)
    dx, dw = grads(False, True)
    bx, bw = grads(True, True)
    assert ew.abs().max() > 0 and dw.abs().max() > 0 and ex.abs().max() > 0 and dx.abs().max() > 0
    assert torch.equal(bx, ex + dx) and torch.equal(bw, ew + dw)
    assert not torch.equal(bw, dw)   # (what the parent commit did: the eikonal term silently missing)


def test_third_order_raises():
    net, x, _ = _module()
    xt = torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = net(xt)
    gx = torch.autograd.grad(y.sum(), xt, create_graph=True)[0]
    d2 = torch.autograd.grad((gx ** 2).sum(), net.weights, create_graph=True)[0]
    assert d2.requires_grad
    with pytest.raises(RuntimeError, match='ffmlp: third-order gradients are not provided'):
        d2.sum().backward()


def test_loss_on_the_weight_gradient_raises():
    net, x, _ = _module()
    xt = torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = net(xt)
    gx, gw = torch.autograd.grad(y.sum(), (xt, net.weights), create_graph=True)
    with pytest.raises(RuntimeError, match='ffmlp: second order with respect to grad_weights is not provided'):
        ((gw ** 2).sum() + (gx ** 2).sum()).backward()


# ---- end to end: hash grid (D 3, L 4, C 2, H 4, 2^8 entries per level) -> 8 features, zero-padded to 16 -> FFMLP(16 -> 64 x 3 -> 1) ----

class _GridRestated:
    """float64 pure-PyTorch statement of the encoder (linear interpolation, hash grid), differentiable to any order in x and E, as
    tests/test_gpu_grid_second_order.py states it: the cells and corner entries are the kernels' (from the fp32 position, fma(x, s, 0.5)
    rounded once), the fraction is that fp32 fraction plus s (x - x0) so that autograd sees d frac / dx = s"""

    def __init__(self, enc):
        capi = _capi()
        self.L, self.C, self.H = enc.num_levels, enc.level_dim, enc.base_resolution
        self.S = float(np.log2(enc.per_level_scale))
        self.offsets = enc.offsets
        self.offsets_list = [int(v) for v in enc.offsets.tolist()]
        sc, res = (ctypes.c_float * self.L)(), (ctypes.c_uint32 * self.L)()
        capi.check(capi.lib.ngp_grid_level_table(self.L, ctypes.c_float(self.S), self.H, sc, res))
        self.scales = [float(v) for v in sc]

    def corner_indices(self, x):
        capi = _capi()
        B = x.shape[0]
        idx = torch.empty(self.L, B, 8, dtype=torch.int32, device=DEV)
        capi.check(capi.lib.ngp_grid_corner_indices(capi.ptr(x), capi.ptr(self.offsets), capi.ptr(idx), B, 3, self.L, ctypes.c_float(self.S), self.H,
                                                    0, 0, capi.stream()))
        return idx.to(torch.int64) & 0xFFFFFFFF

    def __call__(self, x64, E):
        B = x64.shape[0]
        x0 = x64.detach().float().double()
        idx = self.corner_indices(x0.float().contiguous())
        outs = []
        for l in range(self.L):
            s = self.scales[l]
            p32 = (x0 * s + 0.5).float()
            cell = torch.floor(p32)
            frac = (p32 - cell).double() + (x64 - x0) * s
            tab = E[self.offsets_list[l]:self.offsets_list[l + 1]]
            out = torch.zeros(B, self.C, dtype=torch.float64, device=DEV)
            for k in range(8):
                wgt = torch.ones(B, dtype=torch.float64, device=DEV)
                for d in range(3):
                    wgt = wgt * (frac[:, d] if (k >> d) & 1 else 1.0 - frac[:, d])
                out = out + wgt[:, None] * tab[idx[l, :, k]].double()
            outs.append(out)
        return torch.stack(outs, 1).reshape(B, self.L * self.C)


def _rel(a, ref):
    a, ref = a.double(), ref.double()
    m = ref.abs().max().item()
    return (a - ref).abs().max().item() / (m if m > 0 else 1.0)


def test_eikonal_through_grid_encoder_and_ffmlp_end_to_end():
    """embeddings.grad and weights.grad of an eikonal loss under autocast against the float64 statement differentiated twice.  Bar: the one
    tests/test_gpu_grid_second_order.py holds the fp16 table to -- twice the first-order fp16 error on the same data (here the worst of
    d sdf / dx, d sum(sdf) / d embeddings and d sum(sdf) / d weights)."""
    from ffmlp import FFMLP
    from gridencoder import GridEncoder
    B, din, hid, nl = 256, 16, 64, 3
    gen = torch.Generator().manual_seed(11)
    enc = GridEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=4, log2_hashmap_size=8, per_level_scale=2.0).to(DEV)
    net = FFMLP(din, 1, hid, nl, activation='softplus').to(DEV)
    with torch.no_grad():   # fp16-representable parameters: autocast's half copies are exact
        enc.embeddings.copy_(((torch.rand(enc.embeddings.shape, generator=gen) - 0.5)).half().float())
        net.weights.copy_(net.weights.half().float())
    x = (torch.rand(B, 3, generator=gen) * 1.8 - 0.9).to(DEV)
    pad = lambda f: torch.nn.functional.pad(f, (0, din - f.shape[1]))

    # float64 statement
    grid64 = _GridRestated(enc)
    E64 = enc.embeddings.detach().double().requires_grad_(True)
    W64 = net.weights.detach().double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    mats = [m for m in torch.split(W64, [hid * din] + [hid * hid] * (nl - 1) + [16 * hid])]
    h = pad(grid64((x64 + 1) / 2, E64))
    for l in range(nl):
        h = torch.log(torch.exp(10 * (h @ mats[l].view(hid, -1).T)) + 1) / 10
    sdf64 = (h @ mats[nl].view(16, hid).T)[:, 0]
    gx64 = torch.autograd.grad(sdf64.sum(), x64, create_graph=True)[0]
    fE64, fW64 = torch.autograd.grad(sdf64.sum(), (E64, W64), retain_graph=True)
    dE64, dW64 = torch.autograd.grad(_eikonal(gx64), (E64, W64))
    k = S._pow2_into_half(dE64.abs().max().item())   # loss scale from the reference alone: max |d loss / d embeddings| into (1/4, 1/2]

    # the product under autocast
    xt = x.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.float16):
        sdf = net(pad(enc(xt)))[:, 0]
        gx = torch.autograd.grad(sdf.sum(), xt, create_graph=True)[0]
    fE, fW = torch.autograd.grad(sdf.sum(), (enc.embeddings, net.weights), retain_graph=True)
    (_eikonal(gx) * 2.0 ** k).backward()
    first = {'gx': _rel(gx.detach(), gx64.detach()), 'dE': _rel(fE, fE64), 'dW': _rel(fW, fW64)}
    errs = {'dE': _rel(enc.embeddings.grad, dE64 * 2.0 ** k), 'dW': _rel(net.weights.grad, dW64 * 2.0 ** k)}
    print(f'PARITY end to end: first order {first} second order {errs} (loss scale 2^{k})')
    assert enc.embeddings.grad.abs().max() > 0 and net.weights.grad.abs().max() > 0
    bar = 2 * max(first.values())
    assert bar > 0 and all(e <= bar for e in errs.values()), (errs, first)
