"""Second order through the grid encoder (gridencoder/grid.py _grid_encode_backward, csrc/grid_second.hip): the backward of the first
backward against a float64 pure-PyTorch statement of the encoder differentiated twice by autograd, gradcheck / gradgradcheck with
nondet_tol = 0 on float64 tables, reproducibility, the config-4 shape in fp32 and fp16, the unchanged first order, an eikonal training
step end to end, and the refusal of third order."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _capi():
    import _ngp_capi as capi
    return capi


def _grid():
    from gridencoder import grid
    return grid


class Geometry:
    def __init__(self, D, C, L, H, log2_T, per_level_scale, gridtype, align_corners, interp):
        grid = _grid()
        self.D, self.C, self.L, self.H = D, C, L, H
        self.S = float(np.log2(per_level_scale))
        self.gridtype, self.align_corners, self.interp = gridtype, align_corners, interp
        offs = grid.level_offsets(D, L, per_level_scale, H, log2_T, align_corners)
        self.offsets = torch.from_numpy(offs).to(DEV)
        self.offsets_list = [int(v) for v in offs]
        self.n_entries = self.offsets_list[-1]
        self.per_level_scale = per_level_scale
        sc, res = (ctypes.c_float * L)(), (ctypes.c_uint32 * L)()
        _capi().check(_capi().lib.ngp_grid_level_table(L, ctypes.c_float(self.S), H, sc, res))
        self.scales = [float(v) for v in sc]

    def encode(self, x, E):
        """the product op: x [B,D] fp32 in [0,1], E [n,C] -> [B, L*C]"""
        return _grid().grid_encode(x, E, self.offsets, self.per_level_scale, self.H, x.requires_grad, self.gridtype, self.align_corners,
                                   self.interp)

    def corner_indices(self, x):
        """[L,B,2^D] int64 entry indices inside each level, as the kernels form them (-1: outside)"""
        capi = _capi()
        B = x.shape[0]
        idx = torch.empty(self.L, B, 1 << self.D, dtype=torch.int32, device=DEV)
        capi.check(capi.lib.ngp_grid_corner_indices(capi.ptr(x), capi.ptr(self.offsets), capi.ptr(idx), B, self.D, self.L, ctypes.c_float(self.S),
                                                    self.H, self.gridtype, int(self.align_corners), capi.stream()))
        return idx.to(torch.int64) & 0xFFFFFFFF

    def reference(self, x, E, idx):
        """float64 pure-PyTorch statement of the encoder, differentiable to any order in x and E: the cells and corner entries are the
        kernels' (from the fp32 position, fma(x, s, 0.5) rounded once), the fraction is that fp32 fraction plus s (x - x0) so that
        autograd sees d frac / dx = s; phi = f or f^2 (3 - 2 f)"""
        B, D, C = x.shape[0], self.D, self.C
        x64 = x if x.dtype == torch.float64 else x.double()
        x0 = x64.detach().float().double()   # the fp32 position the kernels see
        inside = ((x0 >= 0) & (x0 <= 1)).all(dim=1)
        outs = []
        for l in range(self.L):
            s = self.scales[l]
            p32 = (x0 * s + (0.0 if self.align_corners else 0.5)).float()   # exact product + 0.5, rounded once: the kernel's fmaf
            cell = torch.floor(p32)
            frac = (p32 - cell).double() + (x64 - x0) * s
            phi = frac * frac * (3.0 - 2.0 * frac) if self.interp == 1 else frac
            tab = E[self.offsets_list[l]:self.offsets_list[l + 1]]
            out = torch.zeros(B, C, dtype=torch.float64, device=DEV)
            for k in range(1 << D):
                w = torch.ones(B, dtype=torch.float64, device=DEV)
                for d in range(D):
                    w = w * (phi[:, d] if (k >> d) & 1 else 1.0 - phi[:, d])
                i = torch.where(inside, idx[l, :, k], torch.zeros_like(idx[l, :, k]))
                out = out + w[:, None] * tab[i].double()
            outs.append(torch.where(inside[:, None], out, torch.zeros_like(out)))
        return torch.stack(outs, 1).reshape(B, self.L * C)


def _points(B, D, gen, edge=True):
    x = torch.rand(B, D, generator=gen, dtype=torch.float32)
    if edge:
        x[0] = 0.0
        x[1] = 1.0
        x[2, 0] = 1.0
        x[3, D - 1] = 0.0
        x[4, 0] = -0.25     # outside
        x[5, D - 1] = 1.5   # outside
    return x.to(DEV)


def _second_order(fn, x, E, g, u, v):
    """d<u, gx> + d<v, gE> with respect to (E, g, x), through create_graph=True of the first backward"""
    x = x.detach().clone().requires_grad_(True)
    E = E.detach().clone().requires_grad_(True)
    g = g.detach().clone().requires_grad_(True)
    y = fn(x, E)
    gx, gE = torch.autograd.grad(y, (x, E), grad_outputs=g, create_graph=True)
    loss = 0.0
    if u is not None:
        loss = loss + (gx.double() * u).sum()
    if v is not None:
        loss = loss + (gE.double() * v).sum()
    dE, dg, dx = torch.autograd.grad(loss, (E, g, x), allow_unused=True)
    z = lambda t, ref: torch.zeros_like(ref) if t is None else t
    return z(dE, E), z(dg, g), z(dx, x)


def _rel(a, ref):
    a, ref = a.double(), ref.double()
    m = ref.abs().max().item()
    return (a - ref).abs().max().item() / (m if m > 0 else 1.0)


CASES = []
for i, (D, C) in enumerate([(d, c) for d in (2, 3, 4, 5) for c in (1, 2, 4, 8)]):
    CASES.append((D, C, i % 2, (i // 2) % 2 == 1, (i // 4 + i) % 2))
CASES += [(3, 2, 0, False, 1), (3, 2, 1, True, 0), (3, 2, 0, True, 1), (2, 4, 1, False, 1)]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('D,C,gridtype,align_corners,interp', CASES)
def test_second_order_matches_autograd_of_a_restatement(D, C, gridtype, align_corners, interp, dtype):
    geo = Geometry(D, C, L=4, H=4, log2_T=8, per_level_scale=2.0, gridtype=gridtype, align_corners=align_corners, interp=interp)
    gen = torch.Generator().manual_seed(1000 * D + 10 * C + 4 * gridtype + 2 * align_corners + interp)
    B = 384
    x = _points(B, D, gen)
    E = ((torch.rand(geo.n_entries, C, generator=gen, dtype=torch.float64) - 0.5)).to(DEV).to(dtype)
    g = (torch.rand(B, geo.L * C, generator=gen, dtype=torch.float64) - 0.5).to(DEV).to(dtype)
    u = (torch.rand(B, D, generator=gen, dtype=torch.float64) - 0.5).to(DEV)
    v = (torch.rand(geo.n_entries, C, generator=gen, dtype=torch.float64) - 0.5).to(DEV)
    idx = geo.corner_indices(x)
    ref_fn = lambda xx, EE: geo.reference(xx, EE, idx)
    tol = 1e-6 if dtype == torch.float64 else 1e-4
    for name, uu, vv in (('u', u, None), ('v', None, v)):
        got = _second_order(geo.encode, x, E, g, uu, vv)
        ref = _second_order(ref_fn, x.double(), E.double(), g.double(), uu, vv)
        for what, a, r in zip(('dE', 'dg', 'dx'), got, ref):
            assert torch.isfinite(a).all(), (name, what)
            err = _rel(a, r)
            assert err <= tol, f'{name}-term {what}: {err:.3e} > {tol:.0e} of max |ref| = {r.abs().max().item():.3e}'
    # the u-terms are not all zero (the comparison checks something): the table and the inputs receive them
    got = _second_order(geo.encode, x, E, g, u, None)
    assert got[0].abs().max() > 0 and got[1].abs().max() > 0 and got[2].abs().max() > 0


def _small_geometry(interp=1):
    return Geometry(3, 2, L=4, H=4, log2_T=6, per_level_scale=2.0, gridtype=0, align_corners=False, interp=interp)


@pytest.mark.parametrize('interp', [0, 1], ids=['linear', 'smoothstep'])
def test_gradcheck_of_the_input_gradient_over_table_and_upstream(interp):
    geo = _small_geometry(interp)
    gen = torch.Generator().manual_seed(7 + interp)
    B = 12
    x = _points(B, 3, gen, edge=False).requires_grad_(True)
    E = (torch.rand(geo.n_entries, 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV).requires_grad_(True)
    v = (torch.rand(B, geo.L * 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV).requires_grad_(True)

    def h(E, v):
        y = geo.encode(x, E)
        return torch.autograd.grad((v * y).sum(), x, create_graph=True)[0]

    # h is bilinear in (E, v): a central difference is exact for any step, up to the fp32 rounding of the input gradient over the step
    assert torch.autograd.gradcheck(h, (E, v), eps=2e-2, atol=1e-3, rtol=1e-3, nondet_tol=0.0)


@pytest.mark.parametrize('x_grad', [True, False], ids=['x_requires_grad', 'x_constant'])
def test_gradgradcheck_of_the_encoder_over_the_table(x_grad):
    # x_constant: no dy_dx, no grad_inputs -- only the v-term d/d grad of the second order runs
    geo = _small_geometry(1)
    gen = torch.Generator().manual_seed(11)
    x = _points(10, 3, gen, edge=False).requires_grad_(x_grad)
    E = (torch.rand(geo.n_entries, 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV).requires_grad_(True)
    assert torch.autograd.gradgradcheck(lambda E: geo.encode(x, E), (E,), eps=1e-3, atol=1e-6, rtol=1e-4, nondet_tol=0.0)


def test_absent_upstream_terms_launch_nothing(monkeypatch):
    """an eikonal loss differentiates grad_inputs only: its backward runs the u-terms and no v-term (no encoder forward, no first
    backward on a zero table); a loss on grad_embeddings alone runs no u-term"""
    import types
    grid = _grid()
    calls = {'forward': 0, 'backward': 0, 'second': 0}
    real = grid._backend, grid.grid_encode_backward_backward

    def count(name, fn):
        def wrapped(*args, **kwargs):
            calls[name] += 1
            return fn(*args, **kwargs)
        return wrapped

    spy = types.SimpleNamespace(grid_encode_forward=count('forward', real[0].grid_encode_forward),
                                grid_encode_backward=count('backward', real[0].grid_encode_backward),
                                grad_total_variation=real[0].grad_total_variation)
    monkeypatch.setattr(grid, '_backend', spy)
    monkeypatch.setattr(grid, 'grid_encode_backward_backward', count('second', real[1]))
    geo = _config4()
    gen = torch.Generator().manual_seed(12)
    B = 1 << 12
    for dtype in (torch.float32, torch.float64):
        x = _points(B, 3, gen, edge=False).requires_grad_(True)
        E = ((torch.rand(geo.n_entries, 2, generator=gen, dtype=torch.float64) - 0.5) * 1e-2).to(DEV).to(dtype).requires_grad_(True)
        y = geo.encode(x, E)
        gx = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
        for k in calls:
            calls[k] = 0
        ((gx.norm(dim=-1) - 1) ** 2).mean().backward()
        assert calls == {'forward': 0, 'backward': 0, 'second': 1}, calls
        assert E.grad is not None and E.grad.abs().max() > 0
        # the reverse: a loss on grad_embeddings alone, with respect to the upstream gradient
        g = torch.rand(B, geo.L * 2, generator=gen, dtype=torch.float64).to(DEV).to(dtype).requires_grad_(True)
        y = geo.encode(x, E)
        gE = torch.autograd.grad(y, E, grad_outputs=g, create_graph=True)[0]
        for k in calls:
            calls[k] = 0
        dg = torch.autograd.grad((gE * gE).sum(), g)[0]
        assert calls['second'] == 0 and calls['forward'] == 1, calls
        assert dg.abs().max() > 0


def test_fp64_double_backward_is_bit_reproducible():
    geo = Geometry(3, 2, L=16, H=16, log2_T=14, per_level_scale=1.5, gridtype=0, align_corners=False, interp=1)
    gen = torch.Generator().manual_seed(3)
    B = 1 << 14
    x = _points(B, 3, gen)
    E = (torch.rand(geo.n_entries, 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV)
    g = (torch.rand(B, geo.L * 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV)
    u = (torch.rand(B, 3, generator=gen, dtype=torch.float64) - 0.5).to(DEV)
    v = (torch.rand(geo.n_entries, 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV)
    a = _second_order(geo.encode, x, E, g, u, v)
    b = _second_order(geo.encode, x, E, g, u, v)
    for t1, t2 in zip(a, b):
        assert torch.equal(t1, t2)
    assert a[0].abs().max() > 0


def _config4():
    per_level_scale = float(np.exp2(np.log2(2048 / 16) / 15))
    return Geometry(3, 2, L=16, H=16, log2_T=19, per_level_scale=per_level_scale, gridtype=0, align_corners=False, interp=0)


def test_config4_fp32_and_fp16_against_fp64():
    geo = _config4()
    gen = torch.Generator().manual_seed(4)
    B = 1 << 16
    x = _points(B, 3, gen, edge=False)
    # table and upstream magnitudes of a training run: d2 enc / dx2 grows with s^2 (2048^2 on the finest level), and the fp16 outputs
    # must stay finite
    E32 = ((torch.rand(geo.n_entries, 2, generator=gen) - 0.5) * 2e-2).to(DEV)
    g32 = (torch.rand(B, geo.L * 2, generator=gen) - 0.5).to(DEV)
    u = ((torch.rand(B, 3, generator=gen, dtype=torch.float64) - 0.5) * 1e-2).to(DEV)

    # fp32 tables: the fp64 run on the same data
    got = _second_order(geo.encode, x, E32, g32, u, None)
    ref = _second_order(geo.encode, x, E32.double(), g32.double(), u, None)
    for what, a, r in zip(('dE', 'dg', 'dx'), got, ref):
        assert _rel(a, r) <= 1e-4, (what, _rel(a, r))

    # fp16 tables under autocast (even C), against fp64 on the fp16 data; bar: twice the first-order fp16 error on the same data
    E16, g16 = E32.half().float(), g32.half()
    xg = x.detach().clone().requires_grad_(True)
    Eg = E16.detach().clone().requires_grad_(True)
    gg = g16.detach().clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.float16):
        y = geo.encode(xg, Eg)
    assert y.dtype == torch.float16
    gx, gE = torch.autograd.grad(y, (xg, Eg), grad_outputs=gg, create_graph=True)
    dE, dg, dx = torch.autograd.grad((gx.double() * u).sum(), (Eg, gg, xg))
    x64 = x.detach().clone().requires_grad_(True)
    E64 = E16.double().requires_grad_(True)
    g64 = g16.double().requires_grad_(True)
    y64 = geo.encode(x64, E64)
    gx64, gE64 = torch.autograd.grad(y64, (x64, E64), grad_outputs=g64, create_graph=True)
    dE64, dg64, dx64 = torch.autograd.grad((gx64.double() * u).sum(), (E64, g64, x64))
    first = max(_rel(gE, gE64), _rel(gx, gx64))
    assert first > 0
    errs = {what: _rel(a, r) for what, a, r in (('dE', dE, dE64), ('dg', dg, dg64), ('dx', dx, dx64))}
    assert all(e <= 2 * first for e in errs.values()), f'fp16 second order {errs} vs 2 x first-order {first:.3e}'


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['fp64', 'fp32'])
def test_first_order_is_unchanged_under_create_graph(dtype):
    geo = _config4()
    gen = torch.Generator().manual_seed(5)
    B = 1 << 14
    x = _points(B, 3, gen).requires_grad_(True)
    E = (torch.rand(geo.n_entries, 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV).to(dtype).requires_grad_(True)
    g = (torch.rand(B, geo.L * 2, generator=gen, dtype=torch.float64) - 0.5).to(DEV).to(dtype)
    y = geo.encode(x, E)
    gx0, gE0 = torch.autograd.grad(y, (x, E), grad_outputs=g, retain_graph=True)
    gx1, gE1 = torch.autograd.grad(y, (x, E), grad_outputs=g, create_graph=True)
    assert gx1.requires_grad and gE1.requires_grad
    assert torch.equal(gx0, gx1.detach())
    if dtype == torch.float64:
        assert torch.equal(gE0, gE1.detach())
    else:   # (fp32 tables scatter with float atomics: the summation order of colliding adds is not defined)
        assert _rel(gE1.detach(), gE0) <= 1e-6


class _SDF(torch.nn.Module):
    def __init__(self, encoder):
        super().__init__()
        self.encoder = encoder
        self.mlp = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Softplus(), torch.nn.Linear(64, 64), torch.nn.Softplus(),
                                       torch.nn.Linear(64, 1))

    def forward(self, x):
        return self.mlp(self.encoder(x))[:, 0]


def _eikonal_grads(model, x, gt):
    x = x.detach().clone().requires_grad_(True)
    sdf = model(x)
    grad_x = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
    loss = (sdf - gt).abs().mean() + 0.1 * ((grad_x.norm(dim=-1) - 1.0) ** 2).mean()
    model.zero_grad()
    loss.backward()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def test_eikonal_step_end_to_end():
    from gridencoder import GridEncoder
    torch.manual_seed(6)
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048).to(DEV)
    with torch.no_grad():
        enc.embeddings.uniform_(-0.05, 0.05)
    model = _SDF(enc).to(DEV)

    geo = Geometry(3, 2, L=16, H=16, log2_T=19, per_level_scale=enc.per_level_scale, gridtype=0, align_corners=False, interp=0)
    assert geo.offsets_list == [int(v) for v in enc.offsets.tolist()]

    class RefEncoder(torch.nn.Module):   # the pure-PyTorch encoder sharing the table, fp64
        def __init__(self, table):
            super().__init__()
            self.embeddings = torch.nn.Parameter(table.detach().double().clone())

        def forward(self, inputs):
            unit = (inputs + 1) / 2   # GridEncoder.forward's mapping, bound = 1
            idx = geo.corner_indices(unit.detach().float().contiguous())
            return geo.reference(unit, self.embeddings, idx)

    ref = _SDF(RefEncoder(enc.embeddings)).to(DEV).double()
    ref.mlp.load_state_dict({k: v.double() for k, v in model.mlp.state_dict().items()})

    gen = torch.Generator().manual_seed(8)
    B = 1 << 14
    x = (torch.rand(B, 3, generator=gen) * 2 - 1).to(DEV)
    gt = (x.norm(dim=-1) - 0.5).detach()
    got = _eikonal_grads(model, x, gt)
    want = _eikonal_grads(ref, x.double(), gt.double())
    for name, g in got.items():
        r = want[name]
        err = _rel(g, r)
        assert err <= 1e-3, f'{name}: {err:.3e}'


def test_third_order_raises():
    geo = _small_geometry(1)
    gen = torch.Generator().manual_seed(9)
    x = _points(32, 3, gen, edge=False).requires_grad_(True)
    E = (torch.rand(geo.n_entries, 2, generator=gen) - 0.5).to(DEV).requires_grad_(True)
    y = geo.encode(x, E)
    gx = torch.autograd.grad(y.sum(), x, create_graph=True)[0]
    dx2 = torch.autograd.grad((gx ** 2).sum(), x, create_graph=True)[0]
    with pytest.raises(RuntimeError, match='third-order gradients are not provided'):
        torch.autograd.grad(dx2.sum(), E)
    gx = torch.autograd.grad(geo.encode(x, E).sum(), x, create_graph=True)[0]
    dx2 = torch.autograd.grad((gx ** 2).sum(), x, create_graph=True)[0]
    with pytest.raises(RuntimeError, match='third-order gradients are not provided'):
        (dx2 ** 2).sum().backward()
