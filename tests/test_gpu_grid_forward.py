"""The grid forward's three kernels (csrc/gridencoder.hip) against the float64 model of tests/grid_forward_cases.py, at the C ABI:
k_grid_forward<T, D, C, true> whenever dy_dx is asked for; without it the scheduled kernels -- k_grid_forward_pair (per-XCD work lists, two
lanes per point, a DPP quad swap) and, for fp16 D = 3 C = 2 without align_corners, k_grid_forward_fast with its dense, power-of-two hashed
and generic bodies.

(a)-(e) run lattice inputs on which the forward has no rounding (the conditions: tests/test_grid_forward_cases.py, on the CPU): a misrouted
corner, a swapped weight, a level read with another level's scale or offset, a tile left out or a row written behind the row count changes
the bits.  (f) runs uniform points on a multi-resolution table against an element-wise rounding bound made from the model alone."""
import ctypes

import numpy as np
import pytest
import torch

import grid_forward_cases as gfc

pytestmark = pytest.mark.gpu

TORCH = {'f16': torch.float16, 'f32': torch.float32}
NUMPY = {'f16': np.float16, 'f32': np.float32}
BITS = {'f16': torch.int16, 'f32': torch.int32}
NGP_ERR_INVALID = 1   # include/ngp_hip.h


def _capi():
    import _ngp_capi as capi
    return capi


def _code(dtype):
    return _capi().NGP_F16 if dtype == 'f16' else _capi().NGP_F32


def _costs(level_cost):
    return None if level_cost is None else ctypes.cast((ctypes.c_float * len(level_cost))(*level_cost), ctypes.c_void_p)


def _forward(entry, x, emb, offs, S, H, C, dtype, gridtype=0, align=False, interp=0, with_dydx=False, bound=0.0, level_cost=None, alt=None,
             parity=None, rows=None, expect=0):
    """one forward call through `entry` into buffers pre-filled with the sentinel; x, emb (and alt), offs: device tensors.
    -> outputs [L, B, C], dy_dx [B, L, D, C] or None (device tensors of the table type)"""
    capi = _capi()
    B, D = x.shape
    L = offs.numel() - 1
    out = torch.empty(L, B, C, device='cuda', dtype=TORCH[dtype])
    out.view(BITS[dtype]).fill_(gfc.SENTINEL[dtype])
    dy = None
    if with_dydx:
        dy = torch.empty(B, L, D, C, device='cuda', dtype=TORCH[dtype])
        dy.view(BITS[dtype]).fill_(gfc.SENTINEL[dtype])
    shape = (B, D, C, L, float(S), H)
    modes = (gridtype, int(align), interp, _code(dtype))
    if entry == 'plain':
        rc = capi.lib.ngp_grid_encode_forward(x.data_ptr(), emb.data_ptr(), offs.data_ptr(), out.data_ptr(), *shape, capi.ptr(dy), *modes, capi.stream())
    elif entry == 'ex':
        rc = capi.lib.ngp_grid_encode_forward_ex(x.data_ptr(), emb.data_ptr(), offs.data_ptr(), out.data_ptr(), *shape, capi.ptr(dy), *modes, bound,
                                                 capi.stream())
    elif entry == 'sched':
        rc = capi.lib.ngp_grid_encode_forward_sched(x.data_ptr(), emb.data_ptr(), offs.data_ptr(), out.data_ptr(), *shape, capi.ptr(dy), *modes, bound,
                                                    _costs(level_cost), capi.stream())
    elif entry == 'sel':
        assert not with_dydx
        rc = capi.lib.ngp_grid_encode_forward_sel(x.data_ptr(), emb.data_ptr(), capi.ptr(alt), capi.ptr(parity), capi.ptr(rows), offs.data_ptr(),
                                                  out.data_ptr(), *shape, *modes, bound, _costs(level_cost), capi.stream())
    else:
        assert entry == 'backend' and bound == 0.0 and level_cost is None
        from gridencoder.backend import _backend
        _backend.grid_encode_forward(x, emb, offs, out, B, D, C, L, S, H, None if dy is None else dy.view(B, L * D * C), gridtype, bool(align), interp)
        rc = 0
    assert rc == expect, (rc, capi.lib.ngp_last_error())
    torch.cuda.synchronize()
    return out, dy


class _Device:
    """a lattice case on the device: points of the pool, table(s), offsets, and the model's bits in the table type"""

    def __init__(self, fc):
        b = fc.base
        self.fc, self.r = fc, gfc.reference(fc)
        T = NUMPY[b.dtype]
        self.pool = torch.from_numpy(np.array(gfc.inputs(fc))).cuda()
        self.emb = torch.from_numpy(np.array(gfc.table(fc))).cuda().to(TORCH[b.dtype])
        self.offs = torch.from_numpy(np.array(self.r['offs'])).cuda()
        self.want_out = torch.from_numpy(self.r['out'].astype(T)).cuda()        # [L, P, C]  (the round trip is exact: the CPU test)
        self.want_dy = torch.from_numpy(self.r['dydx'].astype(T)).cuda()        # [P, L, D, C]
        self.inside = torch.from_numpy(np.array(self.r['inside'])).cuda()
        self.kw = dict(S=self.r['S'], H=b.H, C=b.C, dtype=b.dtype, gridtype=b.gridtype, align=b.align, interp=b.interp)

    def points(self, B):
        idx = torch.from_numpy(gfc.point_index(self.fc, B)).cuda()
        return idx, self.pool.index_select(0, idx).contiguous()

    def run(self, entry, B, x=None, **kw):
        idx, xs = self.points(B)
        return idx, _forward(entry, xs if x is None else x, kw.pop('emb', self.emb), self.offs, **self.kw, **kw)


def _assert_bits(dev, got, want, idx, what, unit, rows=None):
    """got [L, B, C] (or dy_dx [B, L, D, C]) has exactly the bits of the model, gathered from the pool by idx; rows: only these rows count"""
    fc, b = dev.fc, dev.fc.base
    point_axis = 1 if got.dim() == 3 else 0
    want = want.index_select(point_axis, idx)
    if rows is not None:
        got, want = got.narrow(point_axis, 0, rows), want.narrow(point_axis, 0, rows)
    if torch.equal(got.view(BITS[b.dtype]), want.view(BITS[b.dtype])):
        return
    diff = ((got.double() - want.double()) / unit).cpu().numpy()
    bad = np.argwhere((got.view(BITS[b.dtype]) != want.view(BITS[b.dtype])).cpu().numpy())
    bodies = gfc.level_bodies(fc)
    lines = []
    for pos in bad[:8]:
        level, point = (pos[0], pos[1]) if point_axis == 1 else (pos[1], pos[0])
        lines.append('level %d (%s, %d entries) point %d (pool %d) element %s: off by %g units (model %g units)'
                     % (level, bodies[level], b.level_sizes[level], point, int(idx[point]), tuple(int(v) for v in pos[2:]), diff[tuple(pos)],
                        float(want[tuple(pos)]) / unit))
    raise AssertionError('%s, %s, B = %d: %d of %d values differ from the float64 model\n  %s'
                         % (gfc.case_id(fc), what, got.shape[point_axis], len(bad), diff.size, '\n  '.join(lines)))


def _check_three_kernels(fc, entries=('plain',)):
    """(a): the scheduled kernel and the dy_dx kernel give the model's bits, so they agree with each other; outside points give +0"""
    dev = _Device(fc)
    for B in fc.Bs:
        for entry in entries:
            idx, (out, _) = dev.run(entry, B)
            _assert_bits(dev, out, dev.want_out, idx, 'scheduled kernel (%s)' % entry, gfc.out_unit(fc))
            outside = ~dev.inside.index_select(0, idx)
            assert not out.view(BITS[fc.base.dtype])[:, outside].any(), 'outside points encode to +0 at every level'
            idx, (out2, dy) = dev.run(entry, B, with_dydx=True)
            _assert_bits(dev, out2, dev.want_out, idx, 'dy_dx kernel, outputs (%s)' % entry, gfc.out_unit(fc))
            _assert_bits(dev, dy, dev.want_dy, idx, 'dy_dx kernel, dy_dx (%s)' % entry, gfc.dydx_unit(fc))
            assert not dy.view(BITS[fc.base.dtype])[outside].any()
            assert torch.equal(out.view(BITS[fc.base.dtype]), out2.view(BITS[fc.base.dtype]))
    return dev


# (a) exact bits: every (dtype, C, D) | gridtype x align_corners x interpolation over four kinds of level | every tile size, level counts
# around the 8 work lists | batches around a wave and a workgroup step
@pytest.mark.parametrize('fc', gfc.LAYOUT, ids=gfc.case_id)
def test_every_instantiation_is_exact(fc):
    _check_three_kernels(fc)


@pytest.mark.parametrize('fc', gfc.SWEEP, ids=gfc.case_id)
def test_every_index_mode_is_exact_over_four_levels(fc):
    _check_three_kernels(fc)


@pytest.mark.parametrize('fc', gfc.LADDER, ids=gfc.case_id)
def test_every_tile_size_and_level_count_is_exact(fc):
    _check_three_kernels(fc)


@pytest.mark.parametrize('fc', gfc.TINY, ids=gfc.case_id)
def test_tiny_batches_are_exact(fc):
    _check_three_kernels(fc)


# the binding's argument order: three f16 SWEEP cases, each with ONE of gridtype, align_corners and interp set
@pytest.mark.parametrize('fc', [fc for fc in gfc.SWEEP if fc.base.dtype == 'f16' and fc.base.gridtype + int(fc.base.align) + fc.base.interp == 1],
                         ids=gfc.case_id)
def test_backend_binding_is_exact(fc):
    _check_three_kernels(fc, entries=('backend',))


# (b) the in-kernel input mapping: world coordinates 4 x - 2 at bound = 2, the model on the unit lattice
@pytest.mark.parametrize('fc', gfc.MAPPED, ids=gfc.case_id)
def test_input_mapping_is_exact(fc):
    dev = _Device(fc)
    B = fc.Bs[0]
    for entry in ('ex', 'sched'):
        idx, (out, _) = dev.run(entry, B, bound=fc.bound)
        _assert_bits(dev, out, dev.want_out, idx, 'ngp_grid_encode_forward_%s, bound = %g' % (entry, fc.bound), gfc.out_unit(fc))
    # the same world coordinates without the mapping are mostly outside: the mapping is what was tested
    idx, (raw, _) = dev.run('ex', B, bound=0.0)
    assert not torch.equal(raw.view(BITS[fc.base.dtype]), out.view(BITS[fc.base.dtype]))


# (c) a skewed level_cost moves tiles between the XCDs' lists (tests/test_grid_forward_cases.py) and changes no bit
@pytest.mark.parametrize('fc', gfc.COSTS, ids=gfc.case_id)
def test_skewed_costs_are_scheduling_only(fc):
    dev = _Device(fc)
    idx, (out, _) = dev.run('sched', fc.Bs[0], level_cost=fc.level_cost)
    _assert_bits(dev, out, dev.want_out, idx, 'ngp_grid_encode_forward_sched with level costs', gfc.out_unit(fc))
    idx, (plain, _) = dev.run('sched', fc.Bs[0])
    assert torch.equal(out.view(BITS[fc.base.dtype]), plain.view(BITS[fc.base.dtype]))


def _sweep(dtype, gridtype=0, align=False, interp=0):
    return next(fc for fc in gfc.SWEEP if (fc.base.dtype, fc.base.gridtype, fc.base.align, fc.base.interp) == (dtype, gridtype, align, interp))


def _layout(dtype, D, C):
    return next(fc for fc in gfc.LAYOUT if (fc.base.dtype, fc.base.D, fc.base.C) == (dtype, D, C))


# (d) the device-side row count: rows below min(B, rows) carry the model's bits, the rows behind keep the sentinel
@pytest.mark.parametrize('fc', [_sweep('f16'), _sweep('f32'), _layout('f16', 4, 4)], ids=gfc.case_id)
def test_row_count_bounds_the_work(fc):
    dev = _Device(fc)
    B = fc.Bs[0]
    ppb = gfc.launch_ppb(B, len(fc.base.level_sizes))
    bits = BITS[fc.base.dtype]
    for rows in (0, 1, 129, 8 * ppb, B - 1, B, B + 5):
        word = torch.tensor([rows], dtype=torch.int32, device='cuda')   # (a uint32 on the device)
        idx, (out, _) = dev.run('sel', B, rows=word)
        live = min(B, rows)
        if live:
            _assert_bits(dev, out, dev.want_out, idx, 'rows_dev = %d' % rows, gfc.out_unit(fc), rows=live)
        assert bool((out.view(bits)[:, live:] == gfc.SENTINEL[fc.base.dtype]).all()), 'rows_dev = %d: rows behind the count are untouched' % rows


# (e) the double-buffered table: a device word selects the copy (`!= 0`); all three bodies of the fast kernel, and the pair kernel
@pytest.mark.parametrize('fc', [_sweep('f16'), next(fc for fc in gfc.MAPPED if fc.base.D == 2)], ids=gfc.case_id)
def test_parity_selects_the_table(fc):
    assert fc.base.dtype == 'f16'
    dev = _Device(fc)
    B = fc.Bs[0]
    alt = torch.from_numpy(np.array(gfc.table(fc, 1))).cuda().half()
    want_alt = torch.from_numpy(gfc.reference(fc, 1)['out'].astype(np.float16)).cuda()
    assert not torch.equal(want_alt, dev.want_out)
    for value, want in ((0.0, dev.want_out), (1.0, want_alt), (2.0, want_alt)):
        parity = torch.tensor([value], device='cuda')
        idx, (out, _) = dev.run('sel', B, alt=alt, parity=parity, bound=fc.bound)
        _assert_bits(dev, out, want, idx, 'parity = %g' % value, gfc.out_unit(fc))
    idx, (out, _) = dev.run('sel', B, alt=alt, parity=None, bound=fc.bound)
    _assert_bits(dev, out, dev.want_out, idx, 'embeddings_alt without a parity word', gfc.out_unit(fc))


def test_parity_is_refused_for_fp32():
    capi = _capi()
    fc = _sweep('f32')
    dev = _Device(fc)
    alt = dev.emb.clone()
    parity = torch.tensor([1.0], device='cuda')
    _, (out, _) = dev.run('sel', fc.Bs[0], alt=alt, parity=parity, expect=NGP_ERR_INVALID)
    assert capi.lib.ngp_last_error().decode() == 'grid_encode_forward_sel: the double-buffered table is fp16'
    assert bool((out.view(torch.int32) == gfc.SENTINEL['f32']).all()), 'nothing was launched'


# (f) off the lattice: uniform points and the edge rows, 8 levels of per_level_scale 1.3819 from base 16, every index mode, the scheduled
# kernels within the element-wise rounding bound of the float64 model (gfc.off_lattice_case states it)
@pytest.mark.parametrize('D,C,dtype,gridtype,align,interp,bound,log2_size', gfc.OFF_CASES)
def test_off_lattice_within_the_rounding_bound(D, C, dtype, gridtype, align, interp, bound, log2_size):
    oc = gfc.off_lattice_case(D, C, dtype, gridtype, align, interp, bound, log2_size)
    x = torch.from_numpy(np.array(oc['x'])).cuda()
    emb = torch.from_numpy(np.array(oc['emb'])).cuda().to(TORCH[dtype])
    offs = torch.from_numpy(np.array(oc['offs'])).cuda()
    out, _ = _forward('ex', x, emb, offs, oc['S'], oc['H'], C, dtype, gridtype, align, interp, bound=bound)
    got = out.double().cpu().numpy()
    err = np.abs(got - oc['ref'])
    ratio = np.where(oc['tol'] > 0, err / np.where(oc['tol'] > 0, oc['tol'], 1.0), np.where(err > 0, np.inf, 0.0))
    print('max err / bound: %.3g (per level %s); max err %.3g' % (ratio.max(), ' '.join('%.2f' % v for v in ratio.max(axis=(1, 2))), err.max()))
    assert not out.view(BITS[dtype])[:, torch.from_numpy(~oc['inside']).cuda()].any(), 'outside points encode to +0'
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert np.all(err <= oc['tol']), 'level %d (%s) point %d channel %d: err %.3g, bound %.3g' % (
        worst[0], oc['bodies'][worst[0]], worst[1], worst[2], err[worst], oc['tol'][worst])
