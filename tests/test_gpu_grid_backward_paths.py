"""The record-sort grid backward (k_grid_backward_bin, k_grid_backward_accumulate and their host side, csrc/gridencoder.hip) over its paths,
at the smallest batches that take them: equalities that hold BY CONSTRUCTION, bit for bit, with no tolerance -- between two calls, between
the forwarding entries, between the overwriting and the adding flush, between a plan made from the right host offsets and one made from
stale ones.  Tables, inputs and the call are in tests/grid_backward_path_cases.py; T3 is the one table here whose calls have an atomic
level in the sort's launch and use the 512-counter sort kernel."""
import numpy as np
import pytest
import torch

import grid_backward_path_cases as pc
import oracle

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sets(**fields):
    import _ngp_capi as capi
    s = capi.SlabSets()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


@pytest.mark.parametrize('B', pc.BATCHES)
@pytest.mark.parametrize('D,gridtype,align,interp', [(2, 0, False, 0), (2, 1, True, 1), (3, 1, False, 0), (3, 0, True, 0), (3, 0, False, 1), (3, 1, True, 1)])
def test_index_modes_are_reproducible_and_within_the_oracles_budget(D, gridtype, align, interp, B):
    """T1 / T2 over the six index-mode combinations of test_gpu_grid.py::test_backward_binned_all_index_modes, with that test's budget"""
    name = 'T1' if D == 3 else 'T2'
    tab = pc.table(name, align)
    x, g = pc.ray_inputs(name, B)
    kw = dict(gridtype=gridtype, align=align, interp=interp)
    one, two = pc.run(tab, x, g, **kw)['ge'], pc.run(tab, x, g, ws_fill=0x54, **kw)['ge']
    assert _same(one, two)
    got = one.float().cpu().numpy().astype(np.float64)
    ref, _ = oracle.grid_backward(g, x, tab['offs'], int(tab['offs'][-1]), 2, tab['S'], tab['H'], gridtype=gridtype, align_corners=align, interp=interp)
    assert np.all(got[ref == 0] == 0)
    np.testing.assert_allclose(got, ref, rtol=1.5e-3, atol=1e-3 * np.abs(ref).max())
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 6e-4


@pytest.mark.parametrize('B', pc.BATCHES)
@pytest.mark.parametrize('name', ['T1', 'T2', 'T3'])
def test_forwarding_entries_agree_and_found_inf_tells_the_truth(name, B):
    tab = pc.table(name)
    x, g = pc.inputs(name, B)
    base = pc.run(tab, x, g, entry='ws')['ge']
    assert torch.isfinite(base).all() and base.float().abs().sum() > 0
    for entry, found_inf, sets in (('checked', False, None), ('checked', True, None), ('slabs', False, None), ('slabs', True, None),
                                   ('slabs', False, _sets()), ('slabs', True, _sets())):
        out = pc.run(tab, x, g, entry=entry, found_inf=found_inf, sets=sets)
        assert _same(out['ge'], base), (entry, found_inf, sets is not None)
        if found_inf:
            assert float(out['found_inf'][0]) == 0.0
    # one infinite gradient value on the finest (sorted, hashed) level: the flag is raised, and only channel 0 of that sample's corners is not finite
    level, b = tab['L'] - 1, 77
    bad = np.array(g)
    bad[level, b, 0] = np.inf
    corners = oracle.grid_corner_indices(x[b:b + 1], tab['offs'], tab['S'], tab['H'])[level, 0].astype(np.int64) + int(tab['offs'][level])
    poisoned = torch.zeros(base.shape, dtype=torch.bool, device='cuda')
    poisoned[torch.from_numpy(corners).cuda(), 0] = True
    for entry in ('checked', 'slabs'):
        out = pc.run(tab, x, bad, entry=entry, found_inf=True)
        assert float(out['found_inf'][0]) == 1.0
        off = ~torch.isfinite(out['ge'])
        assert off.any() and not (off & ~poisoned).any()
        assert torch.equal(_bits(out['ge'])[~poisoned], _bits(base)[~poisoned])   # everything else keeps its bits


@pytest.mark.parametrize('B', pc.BATCHES)
@pytest.mark.parametrize('name', ['T1', 'T3'])
def test_overwrite_fills_a_nan_table_like_a_plain_call_fills_a_zeroed_one(name, B):
    """T1: every level sorted, the flush stores every entry.  T3: not every level sorted, the table is zeroed first and added to"""
    tab = pc.table(name)
    x, g = pc.inputs(name, B)
    base = pc.run(tab, x, g, entry='ws')['ge']
    nan = torch.full_like(base, float('nan'))
    out = pc.run(tab, x, g, entry='slabs', ge=nan, sets=_sets(overwrite_table=1))
    assert _same(out['ge'], base)
    nan = torch.full_like(base, float('nan'))
    out = pc.run(tab, x, g, entry='slabs', ge=nan, found_inf=True, sets=_sets(overwrite_table=1))
    assert _same(out['ge'], base) and float(out['found_inf'][0]) == 0.0


@pytest.mark.parametrize('B', pc.BATCHES)
def test_scaled_records_are_reproducible(B):
    """gradients x 6000: run sums leave the range of an unscaled record (|sum| >= 32768), so records travel as sum / 64 with the scale flag in
    their key (read back from the workspace here); ten calls give the same bits and no NaN"""
    tab = pc.table('T1')
    x, g = pc.ray_inputs('T1', B, magnitude=6000.0)
    outs = [pc.run(tab, x, g) for _ in range(10)]
    assert all(_same(o['ge'], outs[0]['ge']) for o in outs[1:])
    assert not torch.isnan(outs[0]['ge']).any()
    keys = np.concatenate(pc.record_keys(outs[0]['ws'], [128] * 3 + [8] * 5, B, 3))
    assert len(keys) > B and ((keys & 0x8000) != 0).sum() >= 8 and ((keys & 0x4000) != 0).sum() >= 8, 'the inputs must produce scaled records'


@pytest.mark.parametrize('B', pc.BATCHES)
@pytest.mark.parametrize('size', [16384, 30000])
def test_stale_host_offsets_smaller_device_level(size, B):
    """(a) the device says hashed level 5 of T1 has fewer entries than the host copy the plan was made from (32768: 8 slices): the level fits
    its planned bins and is indexed with the device's size -- the same bits as a plan made from the right offsets"""
    tab = pc.table('T1')
    x, g = pc.ray_inputs('T1', B)
    dev = pc.resized(tab['offs'], 5, size)
    right = pc.run(tab, x, g, offs=dev)['ge']
    stale = pc.run(tab, x, g, offs=dev, host_offs=tab['offs'])['ge']
    assert right.float().abs().sum() > 0 and _same(stale, right)


@pytest.mark.parametrize('B', pc.BATCHES)
def test_stale_host_offsets_level_outgrew_its_bins(B):
    """(b) the device says dense level 0 of T1 (736 entries on the host: 128 round-robin bins) has more than 128 x 4096 entries: its records
    take the atomic -- the same bits as a plan made from the right offsets, in which that level is an atomic level.  Samples on the half lattice
    of level 0: the sums there are exact in any order"""
    tab = pc.table('T1')
    x, g = pc.lattice_inputs('T1', B, 0)
    dev = pc.resized(tab['offs'], 0, pc.DENSE_BINS * pc.SLICE + 8)
    right = pc.run(tab, x, g, offs=dev)['ge']
    stale = pc.run(tab, x, g, offs=dev, host_offs=tab['offs'])['ge']
    assert right[:736].float().abs().sum() > 0 and _same(stale, right)
