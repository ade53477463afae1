"""The inputs of tests/test_gpu_grid_forward.py are what they claim to be (tests/grid_forward_cases.py): conditions on the INPUTS, from the
CPU oracle and the host side of the library alone.  A vacuous case fails here instead of passing there."""
import ctypes

import numpy as np
import pytest

import grid_forward_cases as gfc
import grid_lattice_cases as glc

NUMPY = {'f16': np.float16, 'f32': np.float32}


@pytest.mark.parametrize('fc', gfc.ALL, ids=gfc.case_id)
def test_case_is_exact_and_interpolates(fc):
    b = fc.base
    T = NUMPY[b.dtype]
    r = gfc.reference(fc)
    out_n, dydx_n, cap = gfc.exact_conditions(fc)
    assert out_n <= cap and dydx_n <= cap
    # the table: small integers times 2^-6, both signs, independent columns
    for which in (0, 1):
        j = gfc.table(fc, which).astype(np.float64) * 64
        assert np.array_equal(j, np.rint(j)) and 0.9 * fc.jmax <= np.abs(j).max() <= fc.jmax and j.min() < 0 < j.max()
        assert np.array_equal(gfc.table(fc, which).astype(T).astype(np.float32), gfc.table(fc, which))
    assert not np.array_equal(gfc.table(fc, 0), gfc.table(fc, 1))
    # the float64 model is a multiple of the unit, stays below the cap and survives the round trip through the table type
    for ref, unit in ((r['out'], gfc.out_unit(fc)), (r['dydx'], gfc.dydx_unit(fc))):
        q = ref / unit
        assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= cap
        assert np.array_equal(ref.astype(T).astype(np.float64), ref)
    assert np.abs(r['out'] / gfc.out_unit(fc)).max() <= out_n and np.abs(r['dydx'] / gfc.dydx_unit(fc)).max() <= dydx_n
    assert np.any(r['dydx'] != 0)
    # the points of the largest run: outside points of both kinds, the corners of the cube in the whole pool
    x = r['x'][gfc.point_index(fc, max(fc.Bs))]
    inside = r['inside'][gfc.point_index(fc, max(fc.Bs))]
    assert (~inside).sum() >= 0.03 * len(x)
    assert np.all(r['out'][:, ~r['inside']] == 0) and np.all(r['dydx'][~r['inside']] == 0)
    if max(fc.Bs) >= b.B:
        assert (x == 0).all(1).any() and (x == 1).all(1).any()
        outside = x[~inside]
        assert (outside == np.nextafter(np.float32(1), np.float32(2))).any() and (outside == np.float32(-1e-7)).any()
    # interpolation happens: at least 100 points whose output (level 0, channel 0) differs from every one of their corner values
    gidx, ws, _ = r['levels'][0]
    corner_values = gfc.table(fc).astype(np.float64)[gidx, 0]                       # [P, 2^D]
    mixed = inside & np.all(corner_values[gfc.point_index(fc, max(fc.Bs))] != r['out'][0, gfc.point_index(fc, max(fc.Bs)), 0][:, None], axis=1)
    assert mixed.sum() >= 100, mixed.sum()
    # every level takes part, and the levels differ from one another (a level read from another level's table or scale changes the bits)
    for l in range(len(b.level_sizes)):
        assert np.any(r['out'][l] != 0)
        if l:
            assert not np.array_equal(r['out'][l], r['out'][l - 1])


@pytest.mark.parametrize('fc', gfc.MAPPED, ids=gfc.case_id)
def test_world_coordinates_give_the_unit_reference(fc):
    """the model's `bound` argument on world coordinates reproduces the unit-coordinate model, bit for bit, and keeps outside points outside"""
    b = fc.base
    r = gfc.reference(fc)
    xw = gfc.inputs(fc)
    assert fc.bound == glc.BOUND and not np.array_equal(xw, r['x'])
    back = gfc.unit_inputs(xw, fc.bound)
    assert back.dtype == np.float32 and np.array_equal(back[r['inside']], r['x'][r['inside']])
    assert np.all(np.any((back[~r['inside']] < 0) | (back[~r['inside']] > 1), axis=1))
    out, dydx, _, A = gfc.grid_reference(xw, gfc.table(fc), r['offs'], r['S'], b.H, b.gridtype, b.align, b.interp, bound=fc.bound)
    assert np.array_equal(out, r['out']) and np.array_equal(A, r['A'])


def test_layout_covers_every_instantiation():
    assert len({(fc.base.dtype, fc.base.C, fc.base.D) for fc in gfc.LAYOUT}) == 32
    assert all(len(fc.base.level_sizes) == 1 for fc in gfc.LAYOUT)
    kernels = {gfc.scheduled_kernel(fc.base.dtype, fc.base.D, fc.base.C, fc.base.align) for fc in gfc.LAYOUT}
    assert 'pair' in kernels   # (k_grid_forward_fast: SWEEP, MAPPED, LADDER, TINY)


def test_sweep_and_mapped_reach_every_body_of_the_fast_kernel():
    assert len({(fc.base.dtype, fc.base.gridtype, fc.base.align, fc.base.interp) for fc in gfc.SWEEP}) == 16
    reached = set()
    for fc in gfc.SWEEP + gfc.MAPPED:
        b = fc.base
        if gfc.scheduled_kernel(b.dtype, b.D, b.C, b.align) == 'fast':
            reached |= {(body, bool(b.interp), fc.bound > 0.0) for body in gfc.level_bodies(fc)}
    needed = {(body, smooth, mapped) for body in ('dense', 'hashed_pow2', 'generic') for smooth in (False, True) for mapped in (False, True)
              if not (body == 'generic' and mapped)}
    assert needed <= reached, needed - reached
    # and the pair kernel runs with an InputMap, and at fp16 (3, 2) under align_corners
    assert any(gfc.scheduled_kernel(fc.base.dtype, fc.base.D, fc.base.C, fc.base.align) == 'pair' for fc in gfc.MAPPED)
    assert any(fc.base.dtype == 'f16' and fc.base.align and gfc.level_bodies(fc) == ['pair'] * 4 for fc in gfc.SWEEP)


def test_level_bodies_of_known_levels():
    """the restatement of LevelIndexer::init and of the fast kernel's body selection on levels whose body is known from the code's comments"""
    body = lambda size, gridtype, res: gfc.level_body('f16', 3, 2, gridtype, False, size, res)
    assert body(4920, 0, 16) == 'dense' and body(1 << 19, 0, 2048) == 'hashed_pow2' and body(1000, 0, 17) == 'generic'
    assert body(8, 0, 17) == 'hashed_pow2' and body(8, 1, 17) == 'generic' and body(1024, 1, 17) == 'generic' and body(5832, 1, 17) == 'dense'
    assert gfc.level_body('f32', 3, 2, 0, False, 4920, 16) == 'pair' and gfc.level_body('f16', 3, 2, 0, True, 4920, 16) == 'pair'
    ix = gfc.level_indexer(3, 0, True, 4920, 17)
    assert ix.stride == (1, 17, 289) and not ix.hashed and ix.need_mod and ix.mask == 0
    assert gfc.level_indexer(5, 0, False, 1 << 19, 1024).stride == (1, 1025, 0, 0, 0) and gfc.level_indexer(5, 0, False, 1 << 19, 1024).hashed


def test_ladder_reaches_every_tile_size():
    L32 = [fc for fc in gfc.LADDER if len(fc.base.level_sizes) == 32]
    for dtype in ('f16', 'f32'):
        grp = [fc for fc in L32 if fc.base.dtype == dtype]
        assert {gfc.launch_ppb(B, 32) for fc in grp for B in fc.Bs} == {128, 256, 512, 1024}
        for ppb in (256, 512, 1024):
            Bs = sorted(B for fc in grp for B in fc.Bs if gfc.launch_ppb(B, 32) == ppb)
            assert len(Bs) == 2 and gfc.launch_ppb(Bs[0] - 1, 32) == ppb // 2, 'the smallest B that selects the tile size'
            assert all(B % ppb == 1 for B in Bs), 'a last tile of one point'
        assert {len(fc.base.level_sizes) for fc in gfc.LADDER if fc.base.dtype == dtype} == {1, 7, 8, 9, 17, 32}
        assert all(set(gfc.level_bodies(fc)) == ({'dense', 'hashed_pow2', 'generic'} if dtype == 'f16' else {'pair'}) for fc in grp)
    Bs = {B for fc in gfc.TINY + gfc.LADDER for B in fc.Bs}
    assert any(B % 32 == 1 and B > 1 for B in Bs) and any(B % 256 == 1 and B > 1 for B in Bs)
    assert set(gfc.TINY_BS) <= Bs


def _work_lists(L, tiles, costs):
    import _ngp_capi as capi
    lev, t0, end = (ctypes.c_uint16 * 64)(), (ctypes.c_uint32 * 64)(), (ctypes.c_uint32 * 64)()
    arr = None if costs is None else ctypes.cast((ctypes.c_float * L)(*costs), ctypes.c_void_p)
    n = capi.lib.ngp_grid_forward_work_lists(L, tiles, arr, ctypes.cast(lev, ctypes.c_void_p), ctypes.cast(t0, ctypes.c_void_p),
                                             ctypes.cast(end, ctypes.c_void_p))
    return n, list(lev), list(t0), list(end)


@pytest.mark.parametrize('fc', gfc.COSTS, ids=gfc.case_id)
def test_skewed_costs_move_tiles(fc):
    L, B = len(fc.base.level_sizes), fc.Bs[0]
    tiles = -(-B // gfc.launch_ppb(B, L))
    plain, skewed = _work_lists(L, tiles, None), _work_lists(L, tiles, fc.level_cost)
    assert plain[0] > 0 and skewed[0] > 0 and plain != skewed
    assert sum(1 for l in skewed[1] if l == L - 1) > 1, 'the costly level is split over several lists'


@pytest.mark.parametrize('D,C,dtype,gridtype,align,interp,bound,log2_size', gfc.OFF_CASES)
def test_off_lattice_cases(D, C, dtype, gridtype, align, interp, bound, log2_size):
    oc = gfc.off_lattice_case(D, C, dtype, gridtype, align, interp, bound, log2_size)
    assert oc['x'].shape == (gfc.OFF_B, D) and len(oc['offs']) == gfc.OFF_L + 1
    assert (~oc['inside']).sum() == 2 and np.all(oc['ref'][:, ~oc['inside']] == 0) and np.all(oc['tol'] >= 0)
    assert np.all(oc['A'] >= np.abs(oc['ref'])) and np.abs(oc['ref']).max() > 0.1
    if log2_size == 15:
        assert {'dense', 'hashed_pow2'} <= set(oc['bodies'])
    # the bound is a rounding bound: far below the values it guards
    assert np.median(oc['tol'][:, oc['inside']] / np.maximum(np.abs(oc['ref'][:, oc['inside']]), 1e-3)) < (2e-3 if dtype == 'f16' else 2e-5)


def test_off_lattice_cases_cover_what_they_list():
    for dtype in ('f16', 'f32'):
        assert {(c[3], c[4], c[5]) for c in gfc.OFF_CASES if c[:3] == (3, 2, dtype) and c[6:] == (0.0, 12)} >= set(gfc.OFF_MODES)
    assert {(c[0], c[1]) for c in gfc.OFF_CASES} == {(3, 2), (2, 2), (3, 4), (4, 2), (5, 1), (3, 8)}
    assert sum(1 for c in gfc.OFF_CASES if c[6] > 0 and c[7] == 12) == 1
