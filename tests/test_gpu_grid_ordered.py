"""The ordered scatter of the grid encoder's table gradient on the GPU (csrc/grid_ordered.hip): bit for bit against the numpy
model of its order (tests/grid_ordered_cases.py) on lattice inputs, within the rounding bound of the float64 terms on general inputs, the
other outputs unchanged, and the module / determinism-switch / graph-capture routes to it.

The bound of the general-input cases is grid_ordered_cases.bound: (n_e + D + 2) 2^-24 sum|c_i| per entry against the float64 terms, for fp16
tables plus 2^-11 |result| -- stated as 2^-25 where the result lies below fp16's normal range, where the format's spacing no longer
shrinks with the value (measured there: an error of 2.4e-8 = 0.4 of that spacing on a sum of -3.8e-6)."""
import numpy as np
import pytest
import torch

import grid_backward_path_cases as gbp
import grid_ordered_cases as goc

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _mods():
    from gridencoder import backend, grid
    return backend, grid


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def _first(tab, x, g, dtype, with_inputs=False, ordered=True, E=None):
    """the first backward through the ordered entry (or the existing one): -> grad_embeddings [n, C], grad_inputs [B, D] or None"""
    backend, grid = _mods()
    L, B, C = g.shape
    D = tab['D']
    xt, gt, ot = _dev(x), _dev(g, dtype), _dev(tab['offs'])
    n = int(tab['offs'][-1])
    E = torch.zeros(n, C, device=DEV, dtype=dtype) if E is None else E
    dy_dx = gi = None
    if with_inputs:
        out = torch.empty(L, B, C, device=DEV, dtype=dtype)
        dy_dx = torch.empty(B, L * D * C, device=DEV, dtype=dtype)
        backend.grid_encode_forward(xt, E, ot, out, B, D, C, L, tab['S'], tab['H'], dy_dx, tab['gridtype'], tab['align'], tab['interp'])
        gi = torch.zeros(B, D, device=DEV, dtype=dtype)
    ge = torch.zeros(n, C, device=DEV, dtype=dtype)
    fn = backend.grid_encode_backward_ordered if ordered else backend.grid_encode_backward
    fn(gt, xt, E, ot, ge, B, D, C, L, tab['S'], tab['H'], dy_dx, gi, tab['gridtype'], tab['align'], tab['interp'])
    torch.cuda.synchronize()
    return ge, gi


def _second(tab, x, g, u, dtype, E, ordered=True, outputs=True):
    """the second-order backward: -> grad_embeddings, grad_grad, grad_inputs2"""
    backend, grid = _mods()
    L, B, C = g.shape
    D = tab['D']
    xt, gt, ut, ot = _dev(x), _dev(g, dtype), _dev(u, dtype), _dev(tab['offs'])
    ge = torch.zeros(int(tab['offs'][-1]), C, device=DEV, dtype=dtype)
    gg = torch.empty(L, B, C, device=DEV, dtype=dtype) if outputs else None
    gx = torch.empty(B, D, device=DEV, dtype=dtype) if outputs else None
    fn = backend.grid_encode_backward_backward_ordered if ordered else grid.grid_encode_backward_backward
    fn(gt, xt, E, ot, ut, gg, ge, gx, B, D, C, L, tab['S'], tab['H'], tab['gridtype'], tab['align'], tab['interp'])
    torch.cuda.synchronize()
    return ge, gg, gx


def _table_values(tab, dtype, seed=0):
    gen = torch.Generator().manual_seed(77 + seed)
    return (torch.rand(int(tab['offs'][-1]), tab['C'], generator=gen) - 0.5).to(DEV).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('one_cell', [False, True], ids=['B1000', 'one_cell_4133'])
@pytest.mark.parametrize('fp16', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('name', goc.LATTICE_NAMES)
def test_lattice_level_has_the_bits_of_the_model(name, order, fp16, one_cell):
    case = goc.lattice_case(name, order, fp16, one_cell)
    tab, level = case['tab'], case['level']
    dtype, np_dtype = (torch.float16, np.float16) if fp16 else (torch.float32, np.float32)
    if order == 1:
        ge, _ = _first(tab, case['x'], case['g'], dtype)
    else:
        ge, _, _ = _second(tab, case['x'], case['g'], case['u'], dtype, _table_values(tab, dtype), outputs=False)
    want, arrays = goc.ordered_sum(case['keys'], case['contrib'], case['size'], tab['C'], np_dtype)
    assert arrays >= (3 if one_cell else 1)
    lo, hi = int(tab['offs'][level]), int(tab['offs'][level + 1])
    got = ge[lo:hi].cpu().numpy()
    assert np.isfinite(got.astype(np.float64)).all()
    view = np.uint16 if fp16 else np.uint32
    differ = np.argwhere(got.view(view) != want.view(view))
    assert len(differ) == 0, (len(differ), differ[:4].tolist(), got[tuple(differ[0])], want[tuple(differ[0])])


def _check_level_bound(tab, x, g, u, order, level, ge, fp16):
    lo, hi = int(tab['offs'][level]), int(tab['offs'][level + 1])
    keys = goc.record_keys(tab, x, level)
    contrib = goc.contributions(tab, x, g, level, order, u)
    ref, _ = goc.exact_sum(keys, contrib, hi - lo, tab['C'])
    got = ge[lo:hi].cpu().numpy().astype(np.float64)
    limit = goc.bound(keys, contrib, hi - lo, tab['C'], tab['D'], got if fp16 else None)
    err = np.abs(got - ref)
    worst = np.unravel_index(np.argmax(err - limit), err.shape)
    assert (err <= limit).all(), (level, worst, err[worst], limit[worst], ref[worst])


# ---------------------------------------------------------------------------------------------------------------------
# general inputs: every (D, C), both dtypes, the index modes in rotation
# ---------------------------------------------------------------------------------------------------------------------
GENERAL = [(D, C, i % 2, (i // 2) % 2 == 1, (i // 4 + i) % 2) for i, (D, C) in enumerate((d, c) for d in (2, 3, 4, 5) for c in (1, 2, 4, 8))]
B_GENERAL = 257


def _general_inputs(tab, fp16, seed):
    rng = np.random.default_rng(8800 + seed)
    D, L, C = tab['D'], tab['L'], tab['C']
    x = rng.random((B_GENERAL, D), dtype=np.float32)
    x[0], x[1], x[2] = 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))
    x[3, 0] = -1e-7
    x[4:36] = x[36]            # a run of 33 points in one cell
    g = rng.normal(size=(L, B_GENERAL, C)).astype(np.float32)
    u = rng.normal(size=(B_GENERAL, D)).astype(np.float32)
    if fp16:
        g, u = goc.oracle.round_fp16(g), goc.oracle.round_fp16(u)
    return x, g, u


@pytest.mark.parametrize('fp16', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('D,C,gridtype,align,interp', GENERAL)
def test_general_inputs_within_the_rounding_bound_and_reproducible(D, C, gridtype, align, interp, order, fp16):
    tab = goc.general_table(D, C, gridtype, align, interp)
    x, g, u = _general_inputs(tab, fp16, 16 * D + C)
    dtype = torch.float16 if fp16 else torch.float32
    E = _table_values(tab, dtype)
    run = (lambda: _first(tab, x, g, dtype)[0]) if order == 1 else (lambda: _second(tab, x, g, u, dtype, E, outputs=False)[0])
    ge, again = run(), run()
    assert torch.equal(_bits(ge), _bits(again))
    for level in range(tab['L']):
        _check_level_bound(tab, x, g, u, order, level, ge, fp16)


# ---------------------------------------------------------------------------------------------------------------------
# the outputs that were deterministic already
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fp16', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('D,C,gridtype,align,interp', [(2, 2, 0, False, 1), (3, 2, 1, True, 0), (3, 4, 0, False, 1), (4, 2, 0, False, 0), (5, 8, 0, True, 1)])
def test_other_outputs_have_the_bits_of_the_existing_entries(D, C, gridtype, align, interp, fp16):
    tab = goc.general_table(D, C, gridtype, align, interp)
    x, g, u = _general_inputs(tab, fp16, 900 + 16 * D + C)
    dtype = torch.float16 if fp16 else torch.float32
    E = _table_values(tab, dtype)
    ge_o, gi_o = _first(tab, x, g, dtype, with_inputs=True, E=E)
    ge_a, gi_a = _first(tab, x, g, dtype, with_inputs=True, ordered=False, E=E)
    assert torch.equal(_bits(gi_o), _bits(gi_a)) and gi_o.abs().sum() > 0
    assert torch.allclose(ge_o.float(), ge_a.float(), rtol=2e-2 if fp16 else 1e-4, atol=2e-2 if fp16 else 1e-5)
    ge_o, gg_o, gx_o = _second(tab, x, g, u, dtype, E)
    ge_a, gg_a, gx_a = _second(tab, x, g, u, dtype, E, ordered=False)
    assert torch.equal(_bits(gg_o), _bits(gg_a)) and torch.equal(_bits(gx_o), _bits(gx_a))
    assert gg_o.abs().sum() > 0 and gx_o.abs().sum() > 0
    scale = ge_a.float().abs().max().item()
    assert (ge_o.float() - ge_a.float()).abs().max().item() <= (2e-2 if fp16 else 1e-4) * scale


# ---------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------
class _Calls:
    """counts the calls of the two ordered entries (gridencoder.backend, where gridencoder.grid looks them up at each call)"""

    def __init__(self, monkeypatch):
        backend, _ = _mods()
        self.first = self.second = 0
        f, s = backend.grid_encode_backward_ordered, backend.grid_encode_backward_backward_ordered

        def first(*a):
            self.first += 1
            return f(*a)

        def second(*a):
            self.second += 1
            return s(*a)

        monkeypatch.setattr(backend, 'grid_encode_backward_ordered', first)
        monkeypatch.setattr(backend, 'grid_encode_backward_backward_ordered', second)


def _encoder(deterministic, seed=3, **cfg):
    _, grid = _mods()
    cfg = dict(dict(input_dim=3, num_levels=4, level_dim=2, per_level_scale=1.7, base_resolution=4, log2_hashmap_size=9), **cfg)
    enc = grid.GridEncoder(deterministic=deterministic, **cfg).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        enc.embeddings.copy_((torch.rand(enc.embeddings.shape, generator=gen) - 0.5).to(DEV))
    return enc


def _clustered_points(B, D, seed=5):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, D, generator=gen) * 2 - 1
    x[B // 2:] = x[:8].repeat(B, 1)[:B - B // 2] + 1e-3 * torch.rand(B - B // 2, D, generator=gen)   # many points per cell: long runs
    return x.clamp(-1, 1).to(DEV)


def _first_order_grad(enc, x, autocast=False):
    enc.embeddings.grad = None
    gen = torch.Generator().manual_seed(11)
    w = torch.randn(x.shape[0], enc.output_dim, generator=gen).to(DEV)
    with torch.autocast('cuda', dtype=torch.float16, enabled=autocast):
        out = enc(x)
    (out.float() * w).sum().backward()
    torch.cuda.synchronize()
    return enc.embeddings.grad.clone()


def _eikonal_grad(enc, x, autocast=False):
    enc.embeddings.grad = None
    x = x.detach().clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.float16, enabled=autocast):
        sdf = enc(x).float().sum(dim=1)
    (gx,) = torch.autograd.grad(sdf.sum(), x, create_graph=True)
    ((gx.float().norm(dim=1) - 1.0) ** 2).mean().backward()
    torch.cuda.synchronize()
    return enc.embeddings.grad.clone()


def test_module_first_order_fp32_is_reproducible(monkeypatch):
    calls = _Calls(monkeypatch)
    enc, x = _encoder(True), _clustered_points(3000, 3)
    a, b = _first_order_grad(enc, x), _first_order_grad(enc, x)
    assert calls.first == 2 and a.dtype == torch.float32 and a.abs().sum() > 0
    assert torch.equal(_bits(a), _bits(b))
    off = _first_order_grad(_encoder(False), x)
    assert calls.first == 2 and torch.allclose(a, off, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'fp16_autocast'])
def test_module_eikonal_second_order_is_reproducible(monkeypatch, autocast):
    calls = _Calls(monkeypatch)
    enc, x = _encoder(True), _clustered_points(2000, 3)
    a, b = _eikonal_grad(enc, x, autocast), _eikonal_grad(enc, x, autocast)
    assert calls.second == 2 and a.abs().sum() > 0 and torch.isfinite(a).all()
    assert torch.equal(_bits(a), _bits(b))
    off = _eikonal_grad(_encoder(False), x, autocast)
    assert calls.second == 2
    assert (a - off).abs().max().item() <= (3e-2 if autocast else 1e-4) * off.abs().max().item()


def test_determinism_switch_selects_the_ordered_scatter(monkeypatch):
    calls = _Calls(monkeypatch)
    x = _clustered_points(2000, 3)
    forced_first, forced_second = _first_order_grad(_encoder(True), x), _eikonal_grad(_encoder(True), x)
    assert (calls.first, calls.second) == (2, 1)   # (the eikonal step runs the first backward too, as a differentiable op)
    enc = _encoder(None)
    _first_order_grad(enc, x), _eikonal_grad(enc, x)
    assert (calls.first, calls.second) == (2, 1)   # the switch is off: the atomic entries
    torch.use_deterministic_algorithms(True)
    try:
        first, second = _first_order_grad(enc, x), _eikonal_grad(enc, x)
    finally:
        torch.use_deterministic_algorithms(False)
    assert (calls.first, calls.second) == (4, 2)
    assert torch.equal(_bits(first), _bits(forced_first)) and torch.equal(_bits(second), _bits(forced_second))


def test_already_sorted_configuration_keeps_its_path_and_bits(monkeypatch):
    backend, _ = _mods()
    calls = _Calls(monkeypatch)
    cfg, B = gbp.TABLES['T1'], 16384
    x = _dev(gbp.ray_inputs('T1', B)[0]) * 2 - 1
    grads = [_first_order_grad(_encoder(flag, **cfg), x, autocast=True) for flag in (True, False)]
    assert calls.first == 0
    tab = gbp.table('T1')
    assert backend.scatter_path(B, 3, 2, tab['L'], tab['S'], tab['H'], 0, False, torch.float16, True, 1, tab['offs']) == 'sorted'
    assert grads[0].abs().sum() > 0 and torch.equal(_bits(grads[0]), _bits(grads[1]))


def test_ordered_backward_in_a_captured_graph():
    backend, _ = _mods()
    tab, B = gbp.table('T1'), 1000
    x, g = gbp.ray_inputs('T1', B)
    full = dict(tab, C=2, gridtype=0, align=False, interp=0)
    eager, _ = _first(full, x, g, torch.float32)
    xt, gt, ot = _dev(x), _dev(g), _dev(tab['offs'])
    E = torch.zeros(int(tab['offs'][-1]), 2, device=DEV)
    ge = torch.zeros_like(E)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ge.zero_()
        backend.grid_encode_backward_ordered(gt, xt, E, ot, ge, B, 3, 2, tab['L'], tab['S'], tab['H'], None, None, 0, False, 0)
    for _ in range(2):
        ge.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(ge), _bits(eager)) and ge.abs().sum() > 0
