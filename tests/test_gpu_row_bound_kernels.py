"""GPU: every kernel that takes the row bound of the training chain (include/ngp_hip.h ngp_training_row_bound; csrc/common.h live_rows:
live = min(M, word rounded up to 512)), called with a device word w armed and with nothing armed.

What the two calls see.  Below `live` the same inputs, with the zeros the chain defines between w and live (the march zeroes positions and
directions there, the compositor the gradients).  Behind `live` the unbounded call sees what it sees in training today -- finite activations
and ZERO gradient rows, which add nothing to a weight or table gradient -- and the bounded call sees NaN in every input it has no business
reading.  Outputs are prefilled with NaN.  Required: output rows < live are the unbounded call's bits, output rows >= live keep the NaN,
and weight-gradient slabs, reduced gradients, the table gradient, found_inf and (Adam form) both buffer sets of table, moments and fp16
shadow are equal by value (-0 == +0, NaNs in the same places; a difference that is only the sign of a zero is printed with its position)."""
import ctypes

import numpy as np
import pytest
import torch

import grid_backward_path_cases as G
import oracle

pytestmark = pytest.mark.gpu

NAN = float('nan')
NL_S, NL_C = 2, 3                      # the networks of the training step: the paired kernel's NHM = 1 and NHM = 2 forms
EDGE_WORDS = (0, 1, 31, 32, 33, 2048, 4095, 4096, 5000)


def _capi():
    import _ngp_capi as capi
    return capi


def live_rows(M, w):
    return min(M, (min(w, M) + 511) // 512 * 512)


def word(w):
    return torch.tensor([w], dtype=torch.int64).to(torch.int32).cuda()   # a uint32 device word


def p(t):
    return None if t is None else t.data_ptr()


def n_params(nl):
    return 64 * (32 + 64 * (nl - 1) + 16)


def same_bits(a, b):
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def same_values(a, b, what, report):
    """equal by value: -0 == +0, NaNs in the same places; zeros of the other sign go to `report`"""
    af, bf = a.double().flatten(), b.double().flatten()
    na, nb = torch.isnan(af), torch.isnan(bf)
    assert torch.equal(na, nb), f'{what}: NaNs in other places'
    differs = (af != bf) & ~na
    assert not bool(differs.any()), f'{what}: {int(differs.sum())} values differ, first at {int(differs.nonzero()[0])}'
    signs = (torch.signbit(af) != torch.signbit(bf)) & ~na
    if bool(signs.any()):
        report.append((what, int(signs.sum()), int(signs.nonzero()[0])))


# ------------------------------------------------------------------------------------------------
# the network: one set of inputs and one unbounded forward per M, shared by every case
# ------------------------------------------------------------------------------------------------
_NET = {}


def _network(M):
    if M not in _NET:
        capi = _capi()
        gen = torch.Generator(device='cuda').manual_seed(7 + M)
        rnd = lambda *shape, s=1.0: (torch.randn(*shape, device='cuda', generator=gen) * s)
        d = dict(M=M, enc=rnd(16, M, 2, s=0.5).half(), dirs=torch.nn.functional.normalize(rnd(M, 3), dim=1).contiguous(),
                 ws=rnd(n_params(NL_S), s=0.15).half(), wc=rnd(n_params(NL_C), s=0.15).half(), g_sigma=rnd(M, s=0.05).contiguous())
        g_out16 = torch.zeros(M, 16, device='cuda', dtype=torch.half)
        g_out16[:, :3] = rnd(M, 3, s=0.05).half()
        d['g_out16'] = g_out16
        d['fwd'] = _forward(d, None)
        for k, v in d['fwd'].items():
            assert bool(torch.isfinite(v.float()).all()), k
        _NET[M] = d
    return _NET[M]


def _forward(d, w, enc=None, dirs=None):
    """ngp_network_forward (training form, stored activations) into NaN-filled outputs; w: the armed word or None"""
    capi = _capi()
    M = d['M']
    o = dict(sigma=torch.full((M,), NAN, device='cuda'), rgb=torch.full((M, 3), NAN, device='cuda'),
             h16=torch.full((M, 16), NAN, device='cuda', dtype=torch.half), color_in=torch.full((M, 32), NAN, device='cuda', dtype=torch.half),
             fb_s=torch.full((NL_S, M, 64), NAN, device='cuda', dtype=torch.half), fb_c=torch.full((NL_C, M, 64), NAN, device='cuda', dtype=torch.half))
    enc = d['enc'] if enc is None else enc
    dirs = d['dirs'] if dirs is None else dirs
    with capi.row_bound(None if w is None else word(w)):
        capi.check(capi.lib.ngp_network_forward(enc.data_ptr(), dirs.data_ptr(), M, M, d['ws'].data_ptr(), d['wc'].data_ptr(), NL_S, NL_C, 1.0, 1,
                                                o['fb_s'].data_ptr(), o['h16'].data_ptr(), o['sigma'].data_ptr(), o['color_in'].data_ptr(),
                                                o['fb_c'].data_ptr(), o['rgb'].data_ptr(), capi.NGP_FF_INPUT_PLANAR, capi.stream()))
    torch.cuda.synchronize()
    return o


def _tiles(fb, M):
    return fb.view(fb.shape[0], M // 32, 2048)    # the stored activations are kept per tile of 32 rows: [layer][tile][2048] halves


def _backward(d, w, lo, recompute, bounded):
    """colour backward with the sigma epilogue -> sigma backward with the planar dL/dx (both deferred) -> the slab reduction.
    lo: rows >= lo carry a zero gradient.  bounded: the word is armed and every input row (tile) >= live(w) is NaN."""
    capi = _capi()
    M, fwd = d['M'], d['fwd']
    live = live_rows(M, w)
    g_out16, g_sigma = d['g_out16'].clone(), d['g_sigma'].clone()
    g_out16[lo:] = 0
    g_sigma[lo:] = 0
    enc, h16, color_in = d['enc'], fwd['h16'], fwd['color_in']
    fb_s, fb_c = (None, None) if recompute else (fwd['fb_s'], fwd['fb_c'])
    if bounded:
        g_out16[live:] = NAN
        g_sigma[live:] = NAN
        enc, h16, color_in = enc.clone(), h16.clone(), color_in.clone()
        enc[:, live:] = NAN
        h16[live:] = NAN
        color_in[live:] = NAN
        if not recompute:
            fb_s, fb_c = fb_s.clone(), fb_c.clone()
            _tiles(fb_s, M)[:, live // 32:] = NAN
            _tiles(fb_c, M)[:, live // 32:] = NAN
    flags = capi.NGP_FF_DEFER_REDUCE | (capi.NGP_FF_RECOMPUTE if recompute else 0)
    n_c, n_s = capi.lib.ngp_ffmlp_backward_slab_count(M, 32, 64, NL_C), capi.lib.ngp_ffmlp_backward_slab_count(M, 32, 64, NL_S)
    assert n_c > 1 and n_s > 1
    scratch_c = torch.full((NL_C, M, 64), NAN, device='cuda', dtype=torch.half)
    scratch_s = torch.full((NL_S, M, 64), NAN, device='cuda', dtype=torch.half)
    o = dict(g_h16=torch.full((M, 16), NAN, device='cuda', dtype=torch.half), g_enc=torch.full((16, M, 2), NAN, device='cuda', dtype=torch.half),
             g_wc=torch.full((n_params(NL_C),), NAN, device='cuda', dtype=torch.half), g_ws=torch.full((n_params(NL_S),), NAN, device='cuda', dtype=torch.half),
             found_inf=torch.zeros(1, device='cuda'))
    st = capi.stream()
    with capi.row_bound(word(w) if bounded else None):
        capi.check(capi.lib.ngp_network_backward_color(g_out16.data_ptr(), color_in.data_ptr(), d['wc'].data_ptr(), p(fb_c), M, NL_C, scratch_c.data_ptr(),
                                                       g_sigma.data_ptr(), h16.data_ptr(), 1.0, o['g_h16'].data_ptr(), o['g_wc'].data_ptr(), flags, st))
        capi.check(capi.lib.ngp_ffmlp_backward_ex(o['g_h16'].data_ptr(), enc.data_ptr(), d['ws'].data_ptr(), p(fb_s), M, 32, 16, 64, NL_S, 0, 6, 1,
                                                  scratch_s.data_ptr(), o['g_enc'].data_ptr(), o['g_ws'].data_ptr(),
                                                  capi.NGP_FF_INPUT_PLANAR | capi.NGP_FF_DX_PLANAR | flags, st))
    torch.cuda.synchronize()
    o['slabs_c'] = scratch_c.view(-1).view(torch.float32)[:n_c * n_params(NL_C)].clone()
    o['slabs_s'] = scratch_s.view(-1).view(torch.float32)[:n_s * n_params(NL_S)].clone()
    capi.check(capi.lib.ngp_ffmlp_reduce_slabs_pair(scratch_c.data_ptr(), n_c, n_params(NL_C), o['g_wc'].data_ptr(), scratch_s.data_ptr(), n_s,
                                                    n_params(NL_S), o['g_ws'].data_ptr(), o['found_inf'].data_ptr(), st))
    torch.cuda.synchronize()
    return o


def _check_backward(M, w, recompute):
    d = _network(M)
    live = live_rows(M, w)
    lo = min(w, M)
    want = _backward(d, w, lo, recompute, bounded=False)
    got = _backward(d, w, lo, recompute, bounded=True)
    report = []
    assert same_bits(got['g_h16'][:live], want['g_h16'][:live]) and same_bits(got['g_enc'][:, :live], want['g_enc'][:, :live]), (M, w)
    assert bool(torch.isnan(got['g_h16'][live:].float()).all()) and bool(torch.isnan(got['g_enc'][:, live:].float()).all()), (M, w)
    assert bool(torch.isfinite(want['g_h16'].float()).all()) and bool(torch.isfinite(want['g_enc'].float()).all())
    for k in ('slabs_c', 'slabs_s', 'g_wc', 'g_ws', 'found_inf'):
        same_values(got[k], want[k], f'{k} (M={M}, w={w})', report)
    assert float(want['found_inf']) == 0.0 and bool(torch.isfinite(want['g_wc'].float()).all())
    if live > 0 and lo > 0:
        assert float(want['g_ws'].float().abs().max()) > 0
    if report:
        print('equal by value; zeros of the other sign (what, count, first index):', report)


# M = 4096: 128 tiles, one per pair stream of the first 32 workgroups -- under a bound most streams are empty and still leave their slab
@pytest.mark.parametrize('recompute', [False, True], ids=['stored', 'recompute'])
@pytest.mark.parametrize('w', EDGE_WORDS)
def test_mlp_backward_bound_edges(w, recompute):
    _check_backward(4096, w, recompute)


# M = 131072: 4 tiles per stream on 1024 pairs; the double / triple buffering sees streams of 3, 2 and 1-2 tiles with a partial last round
@pytest.mark.parametrize('recompute', [False, True], ids=['stored', 'recompute'])
@pytest.mark.parametrize('w', [98304 + 167, 65536, 32768 + 512])
def test_mlp_backward_bound_across_rounds(w, recompute):
    _check_backward(131072, w, recompute)


# ------------------------------------------------------------------------------------------------
# the forward pair: the two kernels whose own device count is exact take the ROUNDED bound when it is armed
# ------------------------------------------------------------------------------------------------
_GRID = {}


def _grid_forward(w, bounded):
    capi = _capi()
    M = 4096
    if not _GRID:
        offs, pls = oracle.grid_offsets(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048)
        gen = torch.Generator(device='cuda').manual_seed(11)
        _GRID.update(offs=torch.from_numpy(offs.astype(np.int32)).cuda(), S=float(np.log2(pls)),
                     emb=(torch.rand(int(offs[-1]), 2, device='cuda', generator=gen) - 0.5).half(),
                     x=(torch.rand(M, 3, device='cuda', generator=gen) * 2 - 1).contiguous())
    g = _GRID
    x = g['x'].clone()
    x[min(w, M):] = 0                        # the march's zero rows
    if bounded:
        x[live_rows(M, w):] = NAN
    enc = torch.full((16, M, 2), NAN, device='cuda', dtype=torch.half)
    with capi.row_bound(word(w) if bounded else None):
        capi.check(capi.lib.ngp_grid_encode_forward_sched(x.data_ptr(), g['emb'].data_ptr(), g['offs'].data_ptr(), enc.data_ptr(), M, 3, 2, 16, g['S'], 16,
                                                          None, 0, 0, 0, capi.NGP_F16, 1.0, None, capi.stream()))
    torch.cuda.synchronize()
    return enc


@pytest.mark.parametrize('w', EDGE_WORDS)
def test_forward_pair_takes_the_rounded_bound(w):
    M = 4096
    live = live_rows(M, w)
    want, got = _grid_forward(w, False), _grid_forward(w, True)
    assert bool(torch.isfinite(want.float()).all())
    assert same_bits(got[:, :live], want[:, :live]) and bool(torch.isnan(got[:, live:].float()).all()), w
    d = _network(M)
    enc, dirs = d['enc'].clone(), d['dirs'].clone()
    enc[:, live:] = NAN
    dirs[live:] = NAN
    base, o = d['fwd'], _forward(d, w, enc, dirs)
    for k, v in o.items():
        if k in ('fb_s', 'fb_c'):
            v, b = _tiles(v, M), _tiles(base[k], M)
            assert same_bits(v[:, :live // 32], b[:, :live // 32]) and bool(torch.isnan(v[:, live // 32:].float()).all()), (w, k)
        else:
            assert same_bits(v[:live], base[k][:live]) and bool(torch.isnan(v[live:].float()).all()), (w, k)
    # its own (exact) device count wins over the armed word: ngp_network_forward_rows / ngp_grid_encode_forward_sel keep their meaning
    capi = _capi()
    sig, rgb = torch.full((M,), NAN, device='cuda'), torch.full((M, 3), NAN, device='cuda')
    with capi.row_bound(word(M)):
        capi.check(capi.lib.ngp_network_forward_rows(d['enc'].data_ptr(), d['dirs'].data_ptr(), M, M, d['ws'].data_ptr(), d['wc'].data_ptr(), NL_S, NL_C, 1.0, 0,
                                                     None, None, sig.data_ptr(), None, None, rgb.data_ptr(), capi.NGP_FF_INPUT_PLANAR, word(w).data_ptr(),
                                                     capi.stream()))
    torch.cuda.synchronize()
    exact = min(M, (w + 31) // 32 * 32)
    assert same_bits(sig[:exact], base['sigma'][:exact]) and bool(torch.isnan(sig[exact:]).all()), w


# ------------------------------------------------------------------------------------------------
# the grid backward: record sort + slice accumulate (T1: every level sorted) and the atomic level that rides in the sort's launch (T3)
# ------------------------------------------------------------------------------------------------
GRID_M = 20480
GRID_WORDS = (0, 1, 511, 512, 513, 16383, 16385, 20479, 20480)


def _grid_backward(name, w, bounded, adam=None):
    capi = _capi()
    tab = G.table(name)
    x, g = G.inputs(name, GRID_M)
    x, g = np.array(x), np.array(g)
    live = live_rows(GRID_M, w)
    g[:, min(w, GRID_M):] = 0.0
    if bounded:
        g[:, live:] = np.nan
        x[live:] = np.nan
    sets = None
    if adam is not None:
        sets = capi.SlabSets()
        sets.overwrite_table = 1
        sets.table_adam = ctypes.cast(ctypes.pointer(adam), ctypes.c_void_p)
    ge = torch.full((int(tab['offs'][-1]), 2), NAN if adam is not None else 0.0, device='cuda', dtype=torch.half)
    with capi.row_bound(word(w) if bounded else None):
        return G.run(tab, x, g, entry='slabs', found_inf=True, sets=sets, ge=ge)


@pytest.mark.parametrize('w', GRID_WORDS)
@pytest.mark.parametrize('name', ['T1', 'T3'])
def test_grid_backward_bound(name, w):
    want, got = _grid_backward(name, w, False), _grid_backward(name, w, True)
    report = []
    same_values(got['ge'], want['ge'], f'table gradient ({name}, w={w})', report)
    same_values(got['found_inf'], want['found_inf'], 'found_inf', report)
    assert float(want['found_inf']) == 0.0 and bool(torch.isfinite(want['ge'].float()).all())
    if w > 0:
        assert float(want['ge'].float().abs().max()) > 0
    if report:
        print('equal by value; zeros of the other sign (what, count, first index):', report)


def _adam_sets(n):
    """a ngp_table_adam_t over fresh buffers: set 0 (the current one, parity 0) random, set 1 NaN"""
    capi = _capi()
    gen = torch.Generator(device='cuda').manual_seed(3)
    bufs = dict(p=[torch.randn(n, 2, device='cuda', generator=gen) * 0.1, torch.full((n, 2), NAN, device='cuda')],
                m=[torch.randn(n, 2, device='cuda', generator=gen) * 1e-3, torch.full((n, 2), NAN, device='cuda')],
                v=[torch.rand(n, 2, device='cuda', generator=gen) * 1e-6, torch.full((n, 2), NAN, device='cuda')],
                h=[torch.full((n, 2), NAN, device='cuda', dtype=torch.half), torch.full((n, 2), NAN, device='cuda', dtype=torch.half)],
                state=torch.tensor([64.0, 0.0, 0.0, 3.0, 1.0, 0.0, 0.0, 0.0], device='cuda'))
    ta = capi.TableAdam()
    for k in range(2):
        ta.param[k], ta.exp_avg[k], ta.exp_avg_sq[k], ta.param_fp16[k] = (bufs[c][k].data_ptr() for c in 'pmvh')
    ta.state = bufs['state'].data_ptr()
    ta.lr, ta.beta1, ta.beta2, ta.eps = 1e-2, 0.9, 0.99, 1e-15
    return ta, bufs


@pytest.mark.parametrize('w', [0, 513, 16385, 20480])
def test_grid_backward_bound_with_the_table_adam(w):
    """the flush of every slice runs whatever the bound -- with 0 live rows the Adam sweep sees a zero gradient, as with all-dead rows today"""
    n = int(G.table('T1')['offs'][-1])
    res = {}
    for bounded in (False, True):
        ta, bufs = _adam_sets(n)
        out = _grid_backward('T1', w, bounded, adam=ta)
        res[bounded] = dict(ge=out['ge'], found_inf=out['found_inf'], **{f'{c}{k}': bufs[c][k] for c in 'pmvh' for k in range(2)})
    report = []
    for k in res[False]:
        same_values(res[True][k], res[False][k], f'{k} (w={w})', report)
    assert float(res[False]['found_inf']) == 0.0
    if report:
        print('equal by value; zeros of the other sign (what, count, first index):', report)
